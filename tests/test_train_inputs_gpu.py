"""GPU: the training batches of the MVPNet baseline built on the device from resident scenes (csrc/train_inputs.hip,
dropin/mvpnet/train_inputs.py). Every stage bit for bit against the NumPy restatement (tests/train_inputs_ref.py): the crop
with its T tries, the resample rule at every size where the kernel takes another path, the frame choice per item, the
unprojection with every flip pattern and the rotation, the whole batch; the reference's own items (fixture g12) through the
crop and, fed its recorded choice, through the later stages; an item with fewer than k valid pixels; the batch through the
real MVPNet3D forward and backward; and no wait for the device. Integers compare equal, floats compare as bits."""
import numpy as np
import pytest
import torch

import scene_inputs_ref as sref
import train_inputs_ref as ref

pytestmark = pytest.mark.gpu

NB_PTS = 256
STRIDE = 1024                                     # MVK_TRAIN_RESAMPLE_STRIDE
CASES = ("c0", "c1", "c2", "c3")


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def ti():
    import mvkpconv
    return mvkpconv.sub("dropin.mvpnet.train_inputs")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same(got, want):
    """A device tensor and a host array of one shape and dtype with the same bytes."""
    got = host(got)
    want = np.asarray(want)
    if got.dtype == np.bool_ or want.dtype == np.bool_:
        got, want = got.astype(np.uint8), want.astype(np.uint8)
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(bits(got), bits(want))


def on_device(scene):
    d = {key: dev(scene[key]) for key in ("points", "seg_label", "images", "poses", "base_point_ind", "pointwise_rgbd_overlap")}
    d["depth"] = dev(np.asarray(scene["depth"]).astype(np.uint16).view(np.int16))
    d["cam_matrix"] = scene["cam_matrix"]
    return d


ON_LO, ON_HI, CENTRE = 18, 19, 17                 # points of scene 1 that lie exactly on a corner of CENTRE's box


@pytest.fixture(scope="module")
def world(ti):
    """Three scenes of different sizes, base points and frame counts. Scene 0 has no labeled point below x = 1.6 (tries
    centred there fail the threshold); scene 1 has two points exactly on the lo and the hi corner of the box of try
    CENTRE."""
    scenes = [ref.synthetic_scene(1, 2000, nf=3, nb=150), ref.synthetic_scene(2, 3100, nf=5, nb=400),
              ref.synthetic_scene(3, 4000, nf=7, nb=333)]
    s0 = scenes[0]
    s0["seg_label"][s0["points"][:, 0] < 1.6] = ref.IGNORE_LABEL
    p = scenes[1]["points"]
    c = p[CENTRE][:2]
    lo = (c - np.float32(0.5) * np.float32(1.5)) - np.float32(0.2)
    hi = (c + np.float32(0.5) * np.float32(1.5)) + np.float32(0.2)
    p[ON_LO, :2], p[ON_HI, :2] = lo, hi
    resident = ti.TrainScenes([on_device(s) for s in scenes])
    offs = np.concatenate([[0], np.cumsum([len(s["points"]) for s in scenes])])
    return dict(scenes=scenes, ts=resident, res=resident.resident, point_off=offs)


def centres_for(world, ids, rng, T=10):
    """[B,T] centres: random ones, with per item kind a try outside the scene (no point), tries in scene 0's unlabeled
    part (below the threshold; all T of them: the fallback), and the try whose box has points on its corners."""
    out = np.zeros((len(ids), T), np.int64)
    for b, s in enumerate(ids):
        pts = world["scenes"][s]["points"]
        out[b] = rng.integers(0, len(pts), T)
        out[b, 0] = (-1, len(pts), 1 << 40)[b % 3]                    # a try with no point
        if s == 0:
            low = np.argsort(pts[:, 0])[:T]                             # below the threshold
            out[b, 1:] = low[1:] if b % 2 == 0 else out[b, 1:]
            out[b, 1] = low[0]
        if s == 1:
            out[b, 1] = CENTRE
    return out


def run_pick(ops, world, ids, centers, **kw):
    sizes = np.array([len(world["scenes"][s]["points"]) for s in ids], np.int64)
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    counts, chosen, box, rows, row_len = ops.train_chunk_pick(world["res"], dev(np.asarray(ids, np.int64)), dev(centers),
                                                              dev(row_off[:-1]), int(row_off[-1]), **kw)
    return counts, chosen, box, rows, row_len, row_off


# ------------------------------------------------------------------------------------------------------------ the crop

@pytest.mark.parametrize("ids", [[1], [1, 1], [0, 1, 2, 1, 0]])
def test_pick_equals_the_restatement(ops, world, ids):
    rng = np.random.default_rng(len(ids))
    centers = centres_for(world, ids, rng)
    counts, chosen, box, rows, row_len, row_off = run_pick(ops, world, ids, centers)
    assert counts.dtype == torch.int32 and chosen.dtype == torch.int32 and box.dtype == torch.float32
    assert rows.dtype == torch.int64 and row_len.dtype == torch.int64
    rows, lens, tries = host(rows), host(row_len), host(chosen)
    seen = set()
    for b, s in enumerate(ids):
        sc = world["scenes"][s]
        w_counts, w_chosen, w_box, w_mask = ref.crop(sc["points"], sc["seg_label"], centers[b])
        assert np.array_equal(host(counts[b]), w_counts), b
        assert tries[b] == w_chosen and same(box[b], w_box), b
        want_row = np.nonzero(w_mask)[0] + world["point_off"][s]
        assert lens[b] == len(want_row) and np.array_equal(rows[row_off[b]:row_off[b] + lens[b]], want_row), b
        assert w_counts[0].tolist() == [0, 0]                           # the try with no point
        seen.add("fallback" if w_chosen < 0 else "try")
        if s == 0:
            assert w_counts[1, 0] > 0 and w_counts[1, 1] / w_counts[1, 0] < 0.3 and w_chosen != 1    # below the threshold
        if s == 1:                                                      # the points on lo and on hi are inside
            assert w_chosen == 1 and {ON_LO, ON_HI} <= set((want_row - world["point_off"][1]).tolist())
            assert np.array_equal(sc["points"][ON_LO, :2], w_box[:2]) and np.array_equal(sc["points"][ON_HI, :2], w_box[2:])
    if len(ids) == 5:
        assert seen == {"fallback", "try"} and tries[0] == -1 and lens[0] == 2000


def test_pick_out_of_range_scene_and_no_tries(ops, world):
    # a scene_id outside the table is an empty item; T = 0 takes the whole scene
    centers = np.zeros((3, 10), np.int64)
    res = world["res"]
    row_off = np.array([0, 100, 200], np.int64)
    counts, chosen, box, rows, row_len = ops.train_chunk_pick(res, dev(np.array([-1, 3, 1 << 40], np.int64)), dev(centers),
                                                              dev(row_off), 300)
    assert not host(counts).any() and host(chosen).tolist() == [-1] * 3 and not host(box).any() and not host(row_len).any()
    counts, chosen, box, rows, row_len = ops.train_chunk_pick(res, dev(np.array([0], np.int64)),
                                                              dev(np.zeros((1, 0), np.int64)), dev(row_off[:1]), 2000)
    sc = world["scenes"][0]
    want = ref.crop(sc["points"], sc["seg_label"], [])
    assert host(chosen).tolist() == [-1] and same(box[0], want[2]) and host(row_len).tolist() == [2000]
    assert np.array_equal(host(rows), np.arange(2000))
    # a row buffer smaller than the chunk: the row is cut to it, nothing is written behind it
    counts, chosen, box, rows, row_len = ops.train_chunk_pick(res, dev(np.array([0], np.int64)),
                                                              dev(np.zeros((1, 0), np.int64)), dev(row_off[:1]), 1500)
    assert host(row_len).tolist() == [1500] and np.array_equal(host(rows), np.arange(1500))


def fixture_world(ti, g12, name):
    c = {key[len(name) + 1:]: v for key, v in g12.items() if key.startswith(name + "/")}
    scene = {"points": c["points"], "seg_label": c["seg_label"], "base_point_ind": c["base_point_ind"],
             "pointwise_rgbd_overlap": c["overlap"], "depth": c["depth"], "images": c["images"], "poses": c["poses"],
             "cam_matrix": c["cam_matrix"]}
    ts = ti.TrainScenes([on_device(scene)])
    return c, dict(scenes=[scene], ts=ts, res=ts.resident, point_off=np.array([0, len(c["points"])]))


@pytest.mark.parametrize("name", CASES)
def test_pick_gives_the_fixtures_try_box_and_row(ops, ti, golden, name):
    c, w = fixture_world(ti, golden("g12_train_chunks"), name)
    counts, chosen, box, rows, row_len, _ = run_pick(ops, w, [0], c["centers"][None])
    n = int(row_len[0])
    assert int(chosen[0]) == int(c["chunk_try"][0]) and same(box[0], c["box"])
    assert n == len(c["row"]) and np.array_equal(host(rows)[:n], c["row"])


# -------------------------------------------------------------------------------------------------------- the resample

RESAMPLE_SIZES = [0, 1, NB_PTS - 1, NB_PTS, NB_PTS + 1, STRIDE - 1, STRIDE, STRIDE + 1, 2 * STRIDE, 3000]


@pytest.mark.parametrize("key_bits", [4, 32])
def test_resample_equals_the_rule_at_every_size(ops, key_bits):
    rng = np.random.default_rng(key_bits)
    rows = [np.sort(rng.choice(10 * nc + 10, nc, replace=False)).astype(np.int64) + 5 for nc in RESAMPLE_SIZES]
    lens = np.array(RESAMPLE_SIZES, np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
    seeds = rng.integers(-(1 << 63), (1 << 63) - 1, len(rows), dtype=np.int64)
    seeds[1] = -1
    sample_rows, sample_pos = ops.train_chunk_resample(dev(np.concatenate(rows)), dev(off), dev(lens), dev(seeds), NB_PTS,
                                                       key_bits=key_bits)
    assert sample_rows.dtype == torch.int64 and sample_pos.dtype == torch.int32 and sample_rows.shape == (len(rows), NB_PTS)
    got_rows, got_pos = host(sample_rows), host(sample_pos)
    ties = 0
    for b, (nc, row) in enumerate(zip(RESAMPLE_SIZES, rows)):
        want = ref.resample_positions(nc, NB_PTS, seeds[b], key_bits)
        assert np.array_equal(got_pos[b], want), nc
        assert np.array_equal(got_rows[b], row[want] if nc else np.full(NB_PTS, -1)), nc
        if nc > NB_PTS:
            assert (np.diff(got_pos[b]) > 0).all()
            keys = ref.keys_of(seeds[b], nc, key_bits)
            taken = np.zeros(nc, bool)
            taken[want] = True
            equal = keys == keys[taken].max()
            ties += int(taken[equal].sum() < equal.sum())
    if key_bits == 4:
        assert ties == sum(nc > NB_PTS for nc in RESAMPLE_SIZES)        # a tie at the threshold in every such row


def test_resample_other_counts_and_a_row_that_leaves_the_buffer(ops):
    row = np.arange(100, 700, dtype=np.int64)
    for nb_pts in (1, 7, 600, 601):
        sample_rows, sample_pos = ops.train_chunk_resample(dev(row), dev(np.array([0], np.int64)), dev(np.array([600], np.int64)),
                                                           dev(np.array([42], np.int64)), nb_pts)
        want = ref.resample_positions(600, nb_pts, 42)
        assert np.array_equal(host(sample_pos[0]), want) and np.array_equal(host(sample_rows[0]), row[want])
    # row_off + row_len past the buffer: cut to it; a negative offset: an empty row
    off, lens = dev(np.array([500, -3], np.int64)), dev(np.array([600, 50], np.int64))
    sample_rows, sample_pos = ops.train_chunk_resample(dev(row), off, lens, dev(np.array([1, 2], np.int64)), 64)
    want = ref.resample_positions(100, 64, 1)
    assert np.array_equal(host(sample_pos[0]), want) and np.array_equal(host(sample_rows[0]), row[500 + want])
    assert (host(sample_pos[1]) == -1).all() and (host(sample_rows[1]) == -1).all()


# ---------------------------------------------------------------------------------------------------- the frame choice

def test_frame_choice_equals_select_frames_of_chunk_per_item(ops, world):
    rng = np.random.default_rng(8)
    ids = [0, 1, 2, 1, 0, 2, 5]                                         # the last one lies outside the table
    rows = []
    for b, s in enumerate(ids[:-1]):
        sc = world["scenes"][s]
        n = len(sc["points"])
        is_base = np.zeros(n, bool)
        is_base[sc["base_point_ind"]] = True
        if b == 3:
            local = np.nonzero(~is_base)[0][::2]                        # a chunk without a base point
        elif b == 4:
            local = np.zeros(0, np.int64)                               # an empty chunk
        elif b == 5:
            local = np.arange(n)
        else:
            local = np.nonzero(rng.random(n) < 0.3)[0]
        rows.append(local.astype(np.int64))
    rows.append(np.arange(10, dtype=np.int64))
    lens = np.array([len(r) for r in rows], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
    flat = np.concatenate([r + (world["point_off"][s] if s < 3 else 0) for r, s in zip(rows, ids)])
    for nv in (1, 3, 9):                                                # 9: more rounds than scene 0 has frames
        sel = ops.train_select_frames(world["res"], dev(np.array(ids, np.int64)), dev(flat), dev(off), dev(lens), nv)
        assert sel.dtype == torch.int32 and sel.shape == (len(ids), nv)
        got = host(sel).tolist()
        for b, s in enumerate(ids[:-1]):
            sc = world["scenes"][s]
            assert got[b] == sref.select_frames_of_chunk(sc["pointwise_rgbd_overlap"], sc["base_point_ind"], rows[b], nv), b
        assert got[3] == got[4] == got[6] == [0] * nv


def test_frame_choice_at_its_capacity(ops, ti):
    # the largest mask (64 KiB of bits: the launch with more than 64 KiB of LDS) beside a small scene
    rng = np.random.default_rng(9)
    nb, n = 524288, 524288 + 1000
    big = {"points": rng.random((n, 3)).astype(np.float32), "seg_label": np.zeros(n, np.int64),
           "base_point_ind": np.sort(rng.choice(n, nb, replace=False)).astype(np.int64),
           "pointwise_rgbd_overlap": rng.random((nb, 4)) < 0.2, "depth": np.zeros((4, 12, 16), np.int16),
           "images": np.zeros((4, 12, 16, 3), np.float32), "poses": np.tile(np.eye(4, dtype=np.float32), (4, 1, 1)),
           "cam_matrix": np.eye(3, dtype=np.float32)}
    small = ref.synthetic_scene(4, 2000, nf=3, nb=70)
    res = ti.TrainScenes([on_device(small), on_device(big)]).resident
    assert res.max_base == nb and res.max_frames == 4
    rows = [np.nonzero(rng.random(n) < 0.5)[0].astype(np.int64), np.nonzero(rng.random(2000) < 0.5)[0].astype(np.int64)]
    lens = np.array([len(r) for r in rows], np.int64)
    flat = np.concatenate([rows[0] + 2000, rows[1]])
    sel = ops.train_select_frames(res, dev(np.array([1, 0], np.int64)), dev(flat), dev(np.array([0, lens[0]], np.int64)),
                                  dev(lens), 3)
    assert host(sel).tolist() == [sref.select_frames_of_chunk(s["pointwise_rgbd_overlap"], s["base_point_ind"], r, 3)
                                  for s, r in ((big, rows[0]), (small, rows[1]))]


def test_resident_set_refuses_scenes_it_cannot_hold(ops, ti, world):
    scene = on_device(ref.synthetic_scene(4, 500, nf=3, nb=70))
    with pytest.raises(ValueError, match="no point or no frame"):
        ti.TrainScenes([dict(scene, points=scene["points"][:0], seg_label=scene["seg_label"][:0])])
    with pytest.raises(ValueError, match="same .h, w."):
        ti.TrainScenes([scene, on_device(ref.synthetic_scene(5, 500, nf=3, nb=70, h=6, w=8))])
    r = world["res"]
    args = (r.points, r.labels, r.base_point_ind, r.bits, r.depth16, r.images, r.poses, r.cam_inv)
    for column, value, word in [(1, 0, "no point"), (5, 0, "no frame"), (0, 5, "overlaps"), (1, 1 << 20, "leaves the buffers"),
                                (6, 1 << 20, "leaves the buffers"), (3, 524289, "524288")]:
        table = r.table_host.copy()
        table[1, column] = value
        with pytest.raises(RuntimeError, match=word):
            ops.TrainResident(*args, table)
    with pytest.raises(RuntimeError, match="labels must be"):
        ops.TrainResident(r.points, r.labels.int(), *args[2:], r.table_host)


# ---------------------------------------------------------------------------------------------------- the unprojection

@pytest.mark.parametrize("with_rot", [False, True])
def test_unprojection_every_flip_pattern_and_the_rotation(ops, ti, world, with_rot):
    from scipy.spatial.transform import Rotation
    ids = [1, 1, 1, 1, 2, 0]
    sel = np.array([[1, 3], [1, 3], [3, 1], [4, 0], [6, 2], [2, 2]], np.int32)     # frame 1 has no valid depth
    flips = np.array([[0, 0], [1, 0], [0, 1], [1, 1], [1, 0], [0, 1]], np.uint8)
    rng = np.random.default_rng(5)
    box = np.stack([ref.crop(world["scenes"][s]["points"], world["scenes"][s]["seg_label"],
                             [int(rng.integers(len(world["scenes"][s]["points"])))], chunk_thresh=0.0)[2] for s in ids])
    angles = rng.uniform(-180, 180, len(ids))
    box[1:4], angles[1:4] = box[0], angles[0]                           # items 0..3 differ in sel and flips only
    rot =np.stack([ti.z_rotation(a) for a in angles]) if with_rot else None
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(
        world["res"], dev(sel), dev(np.array(ids, np.int64)), dev(box), flips=dev(flips),
        rot=dev(rot.reshape(-1, 9)) if with_rot else None)
    assert image_mask.dtype == torch.bool and num_valid.dtype == torch.int32
    some_valid = 0
    for b, s in enumerate(ids):
        w_images, w_keys, w_mask = ref.views(world["scenes"][s], sel[b], box[b], flips[b])
        xyz32 = w_keys.astype(np.float32).reshape(w_mask.shape + (3,))
        w_xyz = ref.rotate(rot[b], xyz32) if with_rot else xyz32
        assert same(keys[b], w_keys) and same(image_xyz[b], w_xyz) and same(image_mask[b], w_mask), b
        assert same(images[b], np.moveaxis(w_images, -1, 1)) and int(num_valid[b]) == int(w_mask.sum()), b
        some_valid += int(w_mask.sum())
        if with_rot:                                                    # the rule is scipy's rotation to within 1 ulp
            apply = Rotation.from_euler("z", angles[b], degrees=True).apply(xyz32.reshape(-1, 3).astype(np.float64))
            ulp = np.spacing(np.abs(apply).astype(np.float32)).astype(np.float64)
            assert (np.abs(w_xyz.reshape(-1, 3).astype(np.float64) - apply) <= ulp).all()
        if sel[b, 0] == 1:
            assert not host(image_mask[b, 0]).any()                     # the frame without valid depth
    assert some_valid > 50
    # a flipped view is the unflipped one mirrored, pixel for pixel
    assert torch.equal(image_xyz[1, 0], image_xyz[0, 0].flip(1)) and torch.equal(images[1, 0], images[0, 0].flip(2))
    assert torch.equal(image_mask[1, 0], image_mask[0, 0].flip(1)) and torch.equal(image_xyz[1, 1], image_xyz[0, 1])


def test_unprojection_of_frames_and_scenes_that_do_not_exist(ops, world):
    ids = np.array([0, 0, 7], np.int64)
    sel = np.array([[3, -1], [0, 1 << 20], [0, 1]], np.int32)           # scene 0 has frames 0..2
    box = np.tile(np.array([-50, -50, 50, 50], np.float32), (3, 1))
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(world["res"], dev(sel), dev(ids), dev(box))
    for b, v in [(0, 0), (0, 1), (1, 1), (2, 0), (2, 1)]:
        assert not host(image_xyz[b, v]).any() and not host(image_mask[b, v]).any() and not host(images[b, v]).any()
        assert not host(keys[b].view(2, -1, 3)[v]).any()
    want = ref.views(world["scenes"][0], [0], box[1])
    assert same(image_mask[1, 0], want[2][0]) and int(num_valid[1]) == int(want[2].sum()) > 0
    assert host(num_valid).tolist()[0] == host(num_valid).tolist()[2] == 0


# ---------------------------------------------------------------------------------------------------------- end to end

FLOAT_KEYS = ("points", "images", "image_xyz")
OTHER_KEYS = ("seg_label", "image_mask", "knn_indices", "chunk_try", "num_valid_pixels")


def restated_batch(ti, world, ids, nv, k, flip, z_rot, seed, tries=10, key_bits=32):
    np.random.seed(seed)
    sizes = [len(world["scenes"][s]["points"]) for s in ids]
    centers, seeds, flips, angles = ti.draw_items(sizes, nv, flip, z_rot, tries)
    items = [ref.item(world["scenes"][s], centers[b], NB_PTS, nv, k, seed=seeds[b],
                      flips=None if flips is None else flips[b], rot=None if angles is None else ti.z_rotation(angles[b]),
                      key_bits=key_bits) for b, s in enumerate(ids)]
    batch = {key: np.stack([np.asarray(it[key]) for it in items]) for key in FLOAT_KEYS + OTHER_KEYS}
    batch["chunk_try"] = batch["chunk_try"].astype(np.int32)
    batch["num_valid_pixels"] = batch["num_valid_pixels"].astype(np.int32)
    return batch, np.random.randint(1 << 30)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("ids", [[2], [0, 1, 2]])
def test_train_chunk_batch_equals_the_restatement(ti, world, ids, nv, k):
    seed = 100 * len(ids) + 10 * nv + k
    want, after_want = restated_batch(ti, world, ids, nv, k, 0.5, (-180, 180), seed)
    np.random.seed(seed)
    got = ti.train_chunk_batch(world["ts"], ids, NB_PTS, nv, k=k, flip=0.5, z_rot=(-180, 180))
    assert np.random.randint(1 << 30) == after_want                     # the same number of draws
    assert set(got) == set(FLOAT_KEYS + OTHER_KEYS)
    for key in FLOAT_KEYS + OTHER_KEYS:
        assert got[key].is_cuda and same(got[key], want[key]), key
    assert got["points"].shape == (len(ids), 3, NB_PTS) and got["knn_indices"].shape == (len(ids), NB_PTS, k)
    assert (got["knn_indices"] >= 0).all() and (got["num_valid_pixels"] >= k).all()


def test_train_chunk_batch_without_augmentation_and_with_short_keys(ti, world):
    ids = [1, 1, 0]
    for kw in (dict(), dict(key_bits=4), dict(tries=3)):
        want, _ = restated_batch(ti, world, ids, 2, 3, 0.0, None, 77, **kw)
        np.random.seed(77)
        got = ti.train_chunk_batch(world["ts"], ids, NB_PTS, 2, **kw)
        assert all(same(got[key], want[key]) for key in FLOAT_KEYS + OTHER_KEYS), kw
    # nine points in ten are labeled nowhere: every try fails and every item is its whole scene
    np.random.seed(77)
    got = ti.train_chunk_batch(world["ts"], ids, NB_PTS, 2, chunk_thresh=0.9)
    assert host(got["chunk_try"]).tolist() == [-1, -1, -1]


@pytest.mark.parametrize("name", CASES)
def test_later_stages_fed_the_recorded_choice_give_the_references_item(ops, ti, golden, name):
    g12 = golden("g12_train_chunks")
    c, w = fixture_world(ti, g12, name)
    nv, k, res = int(g12["nv"]), int(g12["k"]), w["res"]
    sid = dev(np.array([0], np.int64))
    _, chosen, box, rows, row_len, _ = run_pick(ops, w, [0], c["centers"][None])
    sample_rows = dev(c["row"][c["choice"]][None])                      # the reference's crop_pad_choice, not the rule
    zero = dev(np.array([0], np.int64))
    sel = ops.train_select_frames(res, sid, rows, zero, row_len, nv)
    rot = None if np.isnan(c["angle"][0]) else dev(ti.z_rotation(float(c["angle"][0])).reshape(1, 9))
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(res, sel, sid, box, flips=dev(c["flips"][None]), rot=rot)
    offs = dev(np.array([0, NB_PTS], np.int64))
    queries, knn = ops.chunk_knn_many(res.points, sample_rows.view(-1), offs[:1], offs, np.array([NB_PTS]), keys, image_mask, k=k)
    points, seg_label = ops.train_batch_rows(queries, res.labels, sample_rows, rot=rot)
    assert same(points[0], c["out_points"]) and same(seg_label[0], c["out_seg_label"]) and same(images[0], c["out_images"])
    assert same(image_mask[0], c["out_image_mask"]) and same(knn, c["out_knn_indices"])
    # image_xyz: 2 float32 ulp of the largest coordinate (tests/test_train_inputs_cpu.py derives the bound)
    want = c["out_image_xyz"]
    diff = np.abs(host(image_xyz[0]).astype(np.float64) - want.astype(np.float64)).max()
    print("%s: image_xyz differs from the reference by at most %.3g" % (name, diff))
    assert diff <= 2.0 * float(np.spacing(np.float32(np.abs(want).max())))


def test_item_with_fewer_than_k_valid_pixels(ti):
    scene = ref.synthetic_scene(9, 2100, nf=3, nb=100)
    scene["seg_label"][:] = ref.IGNORE_LABEL                            # no try succeeds: the whole scene and its box
    scene["depth"][:] = 0
    scene["depth"][0, 6, 8] = scene["depth"][0, 6, 9] = 1500            # two pixels at the image centre of frame 0
    scene["pointwise_rgbd_overlap"][:] = False
    scene["pointwise_rgbd_overlap"][:, 0] = True
    other = ref.synthetic_scene(11, 2000, nf=4, nb=120)
    ts = ti.TrainScenes([on_device(other), on_device(scene)])
    world = dict(scenes=[other, scene])
    want, _ = restated_batch(ti, world, [1, 0], 1, 3, 0.0, None, 5)
    np.random.seed(5)
    got = ti.train_chunk_batch(ts, [1, 0], NB_PTS, 1, k=3)
    assert all(same(got[key], want[key]) for key in FLOAT_KEYS + OTHER_KEYS)
    counts, knn = host(got["num_valid_pixels"]).tolist(), host(got["knn_indices"])
    assert counts[0] == 2 and counts[1] >= 3 and host(got["chunk_try"])[0] == -1
    assert (knn[0, :, 2] == -1).all() and (np.sort(knn[0, :, :2], axis=1) == [6 * 16 + 8, 6 * 16 + 9]).all()
    assert (knn[1] >= 0).all()


class StandIn2D(torch.nn.Module):
    """Stands for the 2D encoder: {'image': (n,3,h,w)} -> {'feature': (n,c,h,w)}."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def test_batch_through_the_real_network_forward_and_backward(ops, ti, dropin, world):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    torch.manual_seed(3)
    c, n_cls = 8, 20
    net_3d = pn2ssg.PN2SSG(8, n_cls, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().train()
    net = pn2ssg.fuse_training(net, aggregation=True)
    np.random.seed(31)
    batch = ti.train_chunk_batch(world["ts"], [0, 1, 2], NB_PTS, 2, k=3, flip=0.5, z_rot=(-180, 180))
    assert (batch["num_valid_pixels"] >= 3).all() and (batch["knn_indices"] >= 0).all()
    logits = net(batch)["seg_logit"]
    assert logits.shape == (3, n_cls, NB_PTS)
    loss = torch.nn.functional.cross_entropy(logits, batch["seg_label"], ignore_index=-100)
    loss.backward()
    assert torch.isfinite(loss) and (batch["seg_label"] >= 0).any() and (batch["seg_label"] == -100).any()
    grads = [p.grad for p in net.parameters() if p.requires_grad]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(g.abs().max() > 0 for g in grads)
    assert net.net_2d.conv.weight.grad.abs().max() > 0                  # the gradient reaches the encoder through the k-NN
    ops.pn2_check_indices()


def test_train_chunk_batch_never_waits_for_the_device(ti, world):
    def batches():
        np.random.seed(5)
        return [ti.train_chunk_batch(world["ts"], [0, 1, 2], NB_PTS, 2, k=3, flip=0.5, z_rot=(-180, 180)),
                ti.train_chunk_batch(world["ts"], [2], NB_PTS, 1, k=1)]

    warm = batches()                                                    # first use: allocations, the workspace
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
    for g, w in zip(got, warm):
        assert all(torch.equal(g[key], w[key]) for key in w)
