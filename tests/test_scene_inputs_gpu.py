"""GPU: the inputs of the MVPNet whole-scene test built on the device, G chunks at a time (csrc/scene_inputs.hip,
dropin/mvpnet/whole_scene_inputs.py). The frame choice against the NumPy restatement on packed words
(tests/scene_inputs_ref.py), against utils.voting.select_frames chunk by chunk and against the reference's own choices
(fixture g11); the group batches bit for bit against chunk_groups over chunk_rgbd_inputs; the strict box mask on a pixel
that lies exactly on a bound; a chunk with fewer than k valid pixels; predict_whole_scene_rgbd against
predict_whole_scene_grouped; and no wait for the device anywhere in group_rgbd_inputs. Integers compare equal, floats
compare as bits."""
import numpy as np
import pytest
import torch

import chunk_ref
import scene_inputs_ref as ref

pytestmark = pytest.mark.gpu

C20 = 20


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_mvpnet_chunks")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(a, b):
    """Tensors of one shape and dtype with the same bytes (floats compared as bits)."""
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8).reshape(-1),
                                                                     b.contiguous().view(torch.uint8).reshape(-1))


# -------------------------------------------------------------------------------------------------------- frame choice

def chunk_rows(rng, n_points, base_point_ind, G):
    """G ascending, distinct index rows over a scene of n_points: one without any base point, one with every point, one
    whose first and one whose last entry is a base point, random ones behind."""
    is_base = np.zeros(n_points, bool)
    is_base[base_point_ind] = True
    others = np.nonzero(~is_base)[0]
    rows = []
    for g in range(G):
        kind = g % 5
        if kind == 1 and len(others):
            row = others[rng.random(len(others)) < 0.5]                 # no base point (possibly no point at all)
        elif kind == 2:
            row = np.arange(n_points)                                   # all of them
        elif kind == 3:
            b = int(base_point_ind[rng.integers(len(base_point_ind))])  # a base point is the row's FIRST entry
            row = np.concatenate([[b], np.arange(b + 1, n_points)[rng.random(n_points - b - 1) < 0.4]])
        elif kind == 4:
            b = int(base_point_ind[rng.integers(len(base_point_ind))])  # a base point is the row's LAST entry
            row = np.concatenate([np.arange(b)[rng.random(b) < 0.4], [b]])
        else:
            row = np.nonzero(rng.random(n_points) < 0.35)[0]
        rows.append(row.astype(np.int64))
    return rows


def csr_on_device(rows):
    lens = np.array([len(r) for r in rows], np.int64)
    off = np.concatenate([[0], np.cumsum(lens)])[:-1].astype(np.int64)
    flat = np.concatenate(rows + [np.zeros(0, np.int64)]).astype(np.int64)
    return dev(flat), dev(off), dev(lens)


def select_on_device(ops, table, base_point_ind, rows, nv):
    packed = ops.overlap_pack(dev(table))
    want_packed = ref.pack_overlap(table)
    assert packed.dtype == torch.int32 and np.array_equal(host(packed).view(np.uint32), want_packed)
    flat, off, lens = csr_on_device(rows)
    sel = ops.chunk_select_frames(packed, table.shape[0], dev(base_point_ind), flat, off, lens, nv)
    assert sel.dtype == torch.int32 and sel.shape == (len(rows), nv)
    return host(sel).tolist()


def check_selection(ops, dropin, table, base_point_ind, rows, nv):
    voting = dropin("dropin.utils.voting")
    got = select_on_device(ops, table, base_point_ind, rows, nv)
    tab = dev(table)
    for g, row in enumerate(rows):
        assert got[g] == ref.select_frames_of_chunk(table, base_point_ind, row, nv), "chunk %d" % g
        in_chunk = np.isin(base_point_ind, row)
        assert got[g] == voting.select_frames(tab[dev(in_chunk)], nv), "chunk %d" % g
    return got


# nb, nf, nv, density, G: every nb of {1, 31, 32, 33, 64, 65, 400, 6000} (a word, one bit either side of it, two words,
# more than one ballot per wave), every nf of {1, 6, 12, 40, 64, 65, 130} (fewer frames than waves, a wave's lanes and one
# more), nv of 1, 3, 5 and above nf, three densities, G of 1, 3 and 33
SELECT_CASES = [(1, 1, 1, 0.9, 1), (31, 6, 3, 0.3, 3), (32, 12, 5, 0.05, 3), (33, 40, 3, 0.3, 1), (64, 64, 5, 0.9, 3),
                (65, 65, 3, 0.05, 33), (65, 6, 1, 0.3, 33), (400, 130, 5, 0.3, 3), (6000, 40, 3, 0.05, 33),
                (6000, 12, 13, 0.9, 3), (400, 6, 7, 0.3, 1), (31, 1, 3, 0.9, 3)]


@pytest.mark.parametrize("nb, nf, nv, density, G", SELECT_CASES)
def test_frame_choice_equals_restatement_and_select_frames(ops, dropin, nb, nf, nv, density, G):
    rng = np.random.default_rng(nb * 1000 + nf)
    n_points = 3 * nb + 7
    bpi = np.sort(rng.choice(n_points, nb, replace=False)).astype(np.int64)
    table = rng.random((nb, nf)) < density
    got = check_selection(ops, dropin, table, bpi, chunk_rows(rng, n_points, bpi, G), nv)
    assert all(0 <= f < nf for sel in got for f in sel)


def test_frame_choice_ties_exhaustion_and_empty_chunks(ops, dropin):
    rng = np.random.default_rng(3)
    nb, n_points = 70, 200
    bpi = np.sort(rng.choice(n_points, nb, replace=False)).astype(np.int64)
    table = rng.random((nb, 9)) < 0.3
    table[:, 5] = table[:, 2] = table[:, 2] | table[:, 7] | table[:, 1]      # two identical columns that win: the lower one
    everything = [np.arange(n_points, dtype=np.int64)]
    got = check_selection(ops, dropin, table, bpi, everything, 3)
    assert got[0][0] == 2 and 5 not in got[0]
    # nothing to cover at all: frame 0 again and again; so does a chunk without a base point, beside one with all
    assert check_selection(ops, dropin, np.zeros((nb, 9), bool), bpi, everything, 3) == [[0, 0, 0]]
    not_base = np.setdiff1d(np.arange(n_points), bpi)
    got = check_selection(ops, dropin, table, bpi, [not_base, np.zeros(0, np.int64), everything[0]], 4)
    assert got[0] == got[1] == [0, 0, 0, 0] and got[2][0] == 2
    # a chunk that is one point: the first base point, the last base point, a point that is none
    rows = [bpi[:1], bpi[-1:], not_base[:1], np.array([bpi[0], bpi[-1]])]
    got = check_selection(ops, dropin, table, bpi, rows, 2)
    assert got[2] == [0, 0]


@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_frame_choice_gives_the_references_frames(ops, golden, t):
    g11 = golden("g11_unproject_select")
    table, want = g11["table%d" % t], g11["selected%d" % t].tolist()
    nb = table.shape[0]
    bpi = np.arange(nb, dtype=np.int64) * 2 + 1
    rows = [bpi.copy(), np.arange(2 * nb + 1, dtype=np.int64), np.arange(0, 2 * nb, 2, dtype=np.int64)]
    got = select_on_device(ops, table, bpi, rows, len(want))
    assert got[0] == want and got[1] == want and got[2] == [0] * len(want)


def test_frame_choice_at_its_capacity_and_its_refusals(ops):
    # the largest mask (64 KiB of bits) with a few frames, and the most frames; one more of either is refused
    rng = np.random.default_rng(9)
    for nb, nf in [(524288, 4), (400, 4096)]:
        n_points = nb + 1000
        bpi = np.sort(rng.choice(n_points, nb, replace=False)).astype(np.int64)
        table = rng.random((nb, nf)) < 0.2
        rows = [np.arange(n_points, dtype=np.int64), np.nonzero(rng.random(n_points) < 0.5)[0].astype(np.int64)]
        got = select_on_device(ops, table, bpi, rows, 3)
        assert got == [ref.select_frames_of_chunk(table, bpi, r, 3) for r in rows]
    one = torch.zeros(1, dtype=torch.int64, device="cuda")
    for nb, nf, word in [(524289, 1, "524288"), (40, 4097, "4096")]:
        with pytest.raises(RuntimeError, match=word):
            ops.chunk_select_frames(torch.zeros((nf, (nb + 31) // 32), dtype=torch.int32, device="cuda"), nb,
                                    torch.zeros(nb, dtype=torch.int64, device="cuda"), one, one, one, 2)


# ------------------------------------------------------------------------------------------------------- group batches

def frames_on_device(points, **kw):
    return {key: dev(v) if key != "cam_matrix" else v for key, v in ref.synthetic_frames(points, **kw).items()}


def chunks_on_device(dropin, points, thresh):
    cu = dropin("dropin.mvpnet.utils.chunk_util")
    return cu.scene2chunks_legacy(dev(points), chunk_ref.CHUNK_SIZE, chunk_ref.STRIDE, thresh=thresh, margin=chunk_ref.MARGIN,
                                  return_bbox=True)


@pytest.fixture(scope="module")
def scene(dropin, g17):
    """The g17 scene cut into 8 chunks with exactly one below min_nb_pts, synthetic frames (12 x 16, one without depth,
    one with holes), and chunk_rgbd_inputs of every chunk per (nv, k), made once."""
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    p = g17["points"]
    indices, boxes = chunks_on_device(dropin, p, int(g17["thresholds"][2]))
    sizes = sorted(len(i) for i in indices)
    min_nb_pts = sizes[0] + 37
    assert len(indices) == 8 and sizes[0] < min_nb_pts <= sizes[1]
    pts, frames = dev(p), frames_on_device(p)
    cache = {}

    def reference(nv, k):
        if (nv, k) not in cache:
            cache[nv, k] = [tm.chunk_rgbd_inputs(pts, ind, box, frames, nv, k=k) for ind, box in zip(indices, boxes)]
        return cache[nv, k]

    return dict(p=p, pts=pts, labels=dev(g17["labels"]), frames=frames, sf=wsi.SceneFrames(frames), indices=indices,
                boxes=boxes, min_nb_pts=min_nb_pts, reference=reference)


FLOAT_KEYS, OTHER_KEYS = ("points", "images", "image_xyz"), ("image_mask", "knn_indices", "lengths")


def assert_batches_equal(got, want):
    (gb, gi), (wb, wi) = got, want
    assert set(gb) == set(wb) | {"num_valid_pixels"} and set(wb) == set(FLOAT_KEYS + OTHER_KEYS)
    for key in FLOAT_KEYS + OTHER_KEYS:
        assert gb[key].is_cuda and same_bits(gb[key], wb[key]), key
    assert len(gi) == len(wi) and all(a.dtype == torch.int64 and torch.equal(a, b) for a, b in zip(gi, wi))
    nvp = gb["num_valid_pixels"]
    assert nvp.dtype == torch.int32 and torch.equal(nvp.long(), gb["image_mask"].flatten(1).sum(1))


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("G", [1, 2, 3, 32])
def test_group_batches_are_bit_equal_to_chunk_groups(dropin, scene, G, nv, k):
    wg = dropin("dropin.mvpnet.whole_scene_grouped")
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    s = scene
    np.random.seed(4321)
    want = list(wg.chunk_groups(s["reference"](nv, k), G, s["min_nb_pts"], s["pts"].device))
    after_want = np.random.randint(1 << 30)
    np.random.seed(4321)
    got = list(wsi.group_rgbd_inputs(s["pts"], s["indices"], s["boxes"], s["sf"], nv, k=k, chunks_per_forward=G,
                                     min_nb_pts=s["min_nb_pts"]))
    assert np.random.randint(1 << 30) == after_want                     # the same number of draws
    assert len(got) == len(want) == -(-8 // G)
    padded = 0
    for a, b in zip(got, want):
        assert_batches_equal(a, b)
        padded += int((a[0]["lengths"] > torch.tensor([len(i) for i in a[1]], device="cuda")).sum())
        assert (a[0]["knn_indices"] >= 0).all() and a[0]["points"].shape[2] == int(a[0]["lengths"].max())
    assert padded == 1


def test_group_batches_from_numpy_indices(dropin, scene):
    # index vectors that are not views of one device buffer are concatenated once
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    s = scene
    np.random.seed(7)
    want = list(wsi.group_rgbd_inputs(s["pts"], s["indices"], s["boxes"], s["sf"], 2, chunks_per_forward=3,
                                      min_nb_pts=s["min_nb_pts"]))
    np.random.seed(7)
    got = list(wsi.group_rgbd_inputs(s["pts"], [host(i) for i in s["indices"]], s["boxes"], s["sf"], 2, chunks_per_forward=3,
                                     min_nb_pts=s["min_nb_pts"]))
    for (gb, gi), (wb, wi) in zip(got, want):
        assert all(same_bits(gb[key], wb[key]) for key in wb) and all(torch.equal(a, b) for a, b in zip(gi, wi))


def test_pixel_on_the_bound_is_masked_out(ops, dropin, scene):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    s = scene
    frames = dict(s["frames"])
    f = 3
    overlap = torch.zeros_like(frames["pointwise_rgbd_overlap"])
    overlap[:, f] = True                                               # every chunk chooses frame 3 first
    frames["pointwise_rgbd_overlap"] = overlap
    xyz, valid = ops.unproject_depth(frames["depth"][f:f + 1], frames["cam_matrix"], frames["poses"][f:f + 1])
    xyz, valid = host(xyz).reshape(-1, 3), host(valid).reshape(-1)
    ind = s["indices"][0]
    for lower in (True, False):
        for pix in np.argsort(xyz[:, 0])[len(xyz) // 3:]:
            # a box whose widened x bound IS this pixel's float64 x, if the rounding of +- 0.1 allows it
            x0 = xyz[pix, 0]
            edge = x0 + 0.1 if lower else x0 - 0.1
            bound = float(np.float64(edge) - 0.1) if lower else float(np.float64(edge) + 0.1)
            if valid[pix] and bound == x0:
                break
        else:
            pytest.fail("no pixel whose x survives the round trip through the margin")
        y = xyz[:, 1]
        box = np.array([edge, y.min() - 1, 0.0, x0 + 50, y.max() + 1, 1.0]) if lower else \
            np.array([x0 - 50, y.min() - 1, 0.0, edge, y.max() + 1, 1.0])
        bounds = ref.box_bounds(box)
        assert bounds[0 if lower else 1] == x0                          # the equality the strict comparison must see
        want = ref.pixel_mask(xyz, valid, bounds)
        assert not want[pix] and want.any() and (valid & ~want).sum() > 1
        batch, _ = next(wsi.group_rgbd_inputs(s["pts"], [ind], [box], wsi.SceneFrames(frames), 1, k=1, min_nb_pts=1))
        assert host(batch["image_mask"]).reshape(-1).tolist() == want.tolist()
        one = tm.chunk_rgbd_inputs(s["pts"], ind, box, frames, 1, k=1)
        assert torch.equal(batch["image_mask"][0], one["image_mask"]) and same_bits(batch["image_xyz"][0], one["image_xyz"])
        assert int(batch["num_valid_pixels"][0]) == int(want.sum())


# ----------------------------------------------------------------------------------------- too few valid pixels, end to end

class GroupTableModel(torch.nn.Module):
    """Stands for a network that takes 'lengths': returns the next G pre-generated logit tables as [G, C, n_max], NaN
    behind each chunk's own columns (they must not vote), and keeps what it was given."""

    def __init__(self, tables):
        super().__init__()
        self.tables, self.seen, self.modes, self.at = list(tables), [], [], 0

    def forward(self, batch):
        self.modes.append((self.training, torch.is_grad_enabled()))
        self.seen.append(dict(batch))
        if "lengths" not in batch:                                      # predict_whole_scene's call: one chunk
            self.at += 1
            return {"seg_logit": self.tables[self.at - 1].unsqueeze(0)}
        g, n_max = batch["points"].shape[0], batch["points"].shape[2]
        out = torch.full((g, self.tables[0].shape[0], n_max), float("nan"), device="cuda")
        for i in range(g):
            t = self.tables[self.at + i]
            out[i, :, :t.shape[1]] = t
        self.at += g
        return {"seg_logit": out}


def tables_for(scene, seed=5):
    rng = np.random.default_rng(seed)
    return [dev(chunk_ref.table_logits(int(rng.integers(1 << 30)), C20, [max(len(i), scene["min_nb_pts"])])[0])
            for i in scene["indices"]]


def test_chunk_with_fewer_than_k_valid_pixels(ops, dropin, scene):
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    s = scene
    nv, k, bad = 2, 3, 2
    # chunk 2 gets a box a few micrometres wide around one pixel of the frame it chooses first: fewer than 3 valid pixels
    sel = ref.select_frames_of_chunk(host(s["frames"]["pointwise_rgbd_overlap"]), host(s["frames"]["base_point_ind"]),
                                     host(s["indices"][bad]), nv)
    xyz, valid = ops.unproject_depth(s["frames"]["depth"][sel], s["frames"]["cam_matrix"], s["frames"]["poses"][sel])
    xyz, valid = host(xyz).reshape(-1, 3), host(valid).reshape(-1)
    pix = int(np.nonzero(valid)[0][5])
    x0, y0 = xyz[pix, 0], xyz[pix, 1]
    boxes = list(s["boxes"])
    boxes[bad] = np.array([x0 + 0.1 - 1e-6, y0 + 0.1 - 1e-6, 0.0, x0 - 0.1 + 1e-6, y0 - 0.1 + 1e-6, 1.0])
    want_mask = ref.pixel_mask(xyz, valid, ref.box_bounds(boxes[bad]))
    n_valid = int(want_mask.sum())
    assert want_mask[pix] and 1 <= n_valid < k

    def batches(indices, bxs):
        return list(wsi.group_rgbd_inputs(s["pts"], indices, bxs, s["sf"], nv, k=k, chunks_per_forward=1, min_nb_pts=64))

    got = batches(s["indices"], boxes)
    counts = torch.cat([b["num_valid_pixels"] for b, _ in got]).tolist()
    assert counts[bad] == n_valid and all(c >= k for i, c in enumerate(counts) if i != bad)
    rows = host(got[bad][0]["knn_indices"][0])
    assert host(got[bad][0]["image_mask"]).reshape(-1).tolist() == want_mask.tolist()
    assert (rows[:, n_valid:] == -1).all() and want_mask[rows[:, :n_valid]].all()
    assert (np.sort(rows[:, :n_valid], axis=1) == np.nonzero(want_mask)[0]).all()
    # the scene without that chunk: every other chunk's batch is what it was
    keep = [i for i in range(8) if i != bad]
    without = batches([s["indices"][i] for i in keep], [boxes[i] for i in keep])
    for i, (b, ind) in zip(keep, without):
        assert all(same_bits(b[key], got[i][0][key]) for key in b) and torch.equal(ind[0], got[i][1][0])
        assert (b["knn_indices"] >= 0).all()

    # the loop: every group is forwarded, then the scene fails, naming the chunk's count; the evaluator stays untouched
    ev = dropin("dropin.mvpnet.evaluate_3d").Evaluator(["c%d" % i for i in range(C20)])
    model = GroupTableModel(tables_for(s)).train()
    with pytest.raises(ValueError, match="n_samples = %d, n_neighbors = 3" % n_valid):
        wsi.predict_whole_scene_rgbd(model, s["pts"], s["indices"], boxes, s["sf"], nv, k=k, min_nb_pts=s["min_nb_pts"],
                                     seg_label=s["labels"], evaluator=ev, chunks_per_forward=3)
    assert len(model.seen) == 3 and model.training and not ev.confusion_matrix.any()
    assert all((seen["knn_indices"] >= 0).all() for seen in model.seen)  # what the model saw has pixel 0 for "none"


@pytest.mark.parametrize("G", [1, 3, 32])
def test_predict_whole_scene_rgbd_equals_the_grouped_loop(dropin, scene, G):
    wg = dropin("dropin.mvpnet.whole_scene_grouped")
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    Evaluator = dropin("dropin.mvpnet.evaluate_3d").Evaluator
    s = scene
    nv, k = 2, 3
    tables = tables_for(s)
    ev_want, ev_got = (Evaluator(["c%d" % i for i in range(C20)]) for _ in range(2))
    np.random.seed(1234)
    want_pred, want_mean = wg.predict_whole_scene_grouped(GroupTableModel(tables), s["pts"], s["reference"](nv, k),
                                                          min_nb_pts=s["min_nb_pts"], seg_label=s["labels"],
                                                          evaluator=ev_want, chunks_per_forward=G)
    model = GroupTableModel(tables).train()
    np.random.seed(1234)
    pred, mean = wsi.predict_whole_scene_rgbd(model, s["pts"], s["indices"], s["boxes"], s["sf"], nv, k=k,
                                              min_nb_pts=s["min_nb_pts"], seg_label=s["labels"], evaluator=ev_got,
                                              chunks_per_forward=G)
    assert torch.equal(pred, want_pred) and same_bits(mean, want_mean) and not torch.isnan(mean).any()
    assert np.array_equal(ev_got.confusion_matrix, ev_want.confusion_matrix) and ev_got.confusion_matrix.sum() > 0
    assert len(model.seen) == -(-8 // G) and model.training and all(m == (False, False) for m in model.modes)
    assert (pred == C20).any() and (pred < C20).any()


class StandIn2D(torch.nn.Module):
    """Stands for the 2D encoder: {'image': (n,3,h,w)} -> {'feature': (n,c,h,w)}."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def test_predict_whole_scene_rgbd_with_the_real_network(ops, dropin, scene):
    wg = dropin("dropin.mvpnet.whole_scene_grouped")
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    s = scene
    torch.manual_seed(3)
    c, n_cls, k, nv = 8, 5, 3, 2
    net_3d = PN2SSG(8, n_cls, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                    fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    np.random.seed(99)
    want_pred, want_mean = wg.predict_whole_scene_grouped(net, s["pts"], s["reference"](nv, k), min_nb_pts=s["min_nb_pts"],
                                                          chunks_per_forward=3)
    np.random.seed(99)
    pred, mean = wsi.predict_whole_scene_rgbd(net, s["pts"], s["indices"], s["boxes"], s["sf"], nv, k=k,
                                              min_nb_pts=s["min_nb_pts"], chunks_per_forward=3)
    # no point is left unpredicted that the grouped path predicts (the 2D stand-in is a library convolution, whose
    # algorithm may differ from call to call: the logits are not compared here, the inputs are compared as bits above)
    predicted = want_pred < n_cls
    assert predicted.any() and (~predicted).any() and torch.equal(pred < n_cls, predicted)
    assert torch.isfinite(mean).all() and mean.shape == want_mean.shape
    ops.pn2_check_indices()


def test_group_rgbd_inputs_never_waits_for_the_device(dropin, scene):
    wsi = dropin("dropin.mvpnet.whole_scene_inputs")
    s = scene

    def whole_scene(G):
        np.random.seed(5)
        return list(wsi.group_rgbd_inputs(s["pts"], s["indices"], s["boxes"], s["sf"], 2, k=3, chunks_per_forward=G,
                                          min_nb_pts=s["min_nb_pts"]))

    warm = whole_scene(3)                                                # first use: allocations, the workspace
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
            got = whole_scene(3) + whole_scene(1)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    assert len(got) == 3 + 8
    for (gb, _), (wb, _) in zip(got, warm):
        assert all(same_bits(gb[key], wb[key]) for key in wb)
