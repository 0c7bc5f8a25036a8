"""GPU: the MVPNet whole-scene test on the device (csrc/chunk.hip and the drop-in modules mvpnet/utils/chunk_util.py,
mvpnet/evaluate_3d.py, mvpnet/test_mvpnet_3d.py) against the NumPy restatements of tests/chunk_ref.py and the reference's
own outputs (fixture g17). Integers compare equal, floats compare as bits."""
import numpy as np
import pytest
import torch

import chunk_ref
import util

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


def chunks_on_device(dropin, points, thresh, **kw):
    cu = dropin("dropin.mvpnet.utils.chunk_util")
    return cu.scene2chunks_legacy(dev(points), chunk_ref.CHUNK_SIZE, chunk_ref.STRIDE, thresh=thresh, margin=chunk_ref.MARGIN,
                                  return_bbox=True, **kw)


def assert_chunks_equal(got, want):
    (gi, gb), (wi, wb) = got, want
    assert len(gi) == len(wi) and len(gb) == len(wb) == len(wi)
    for a, b in zip(gi, wi):
        assert a.dtype == torch.int64 and a.is_cuda and np.array_equal(host(a), b)
    for a, b in zip(gb, wb):
        assert isinstance(a, np.ndarray) and util.bits_equal(a, np.asarray(b, np.float64))


# ------------------------------------------------------------------------------------------------------------ chunks

@pytest.mark.parametrize("k", [0, 1, 2])
def test_chunks_of_the_dyadic_scene(dropin, g17, k):
    p, t = g17["points"], "t%d/" % k
    thresh = int(chunk_ref.thresholds(p)[k])
    got = chunks_on_device(dropin, p, thresh)
    assert_chunks_equal(got, chunk_ref.scene2chunks(p, thresh=thresh))
    assert len(got[0]) == int(g17[t + "n_chunks"]) and [len(i) for i in got[0]] == g17[t + "sizes"].tolist()
    assert np.array_equal(host(torch.cat(got[0])), g17[t + "indices"])
    assert util.bits_equal(np.asarray(got[1], np.float64), g17[t + "bboxes"])
    # the index vectors are views of one CSR buffer
    base = got[0][0].untyped_storage().data_ptr()
    assert all(i.untyped_storage().data_ptr() == base for i in got[0])


# name, scene, thresh (None: the median of the scene's inner counts), chunks expected (None: some, not all)
SCENES = [("1 m scene: no corner", lambda: chunk_ref.small_scene(3, 777, 1.0), 1, 0),
          ("1.5 m scene: one corner", lambda: chunk_ref.small_scene(4, 3000, 1.5), 100, 1),
          ("one point", lambda: chunk_ref.small_scene(5, 1, 1.0), 1, 0),
          ("two points 1.5 m apart", lambda: chunk_ref.small_scene(6, 2, 1.5), 2, 1),
          ("non-dyadic, 6 000 points", lambda: chunk_ref.random_scene(7, 6000), None, None),
          ("non-dyadic, threshold keeps nothing", lambda: chunk_ref.random_scene(8, 2000), 10 ** 6, 0),
          ("non-dyadic, 70 000 points: 45 workgroups per box", lambda: chunk_ref.random_scene(9, 70000), None, None)]


@pytest.mark.parametrize("name, make, thresh, expected", SCENES, ids=[s[0] for s in SCENES])
def test_chunks_of_other_scenes(ops, dropin, name, make, thresh, expected):
    p = make()
    if thresh is None:
        thresh = chunk_ref.median_threshold(p)
    want = chunk_ref.scene2chunks(p, thresh=thresh)
    if expected is not None:
        assert len(want[0]) == expected
    else:
        assert 0 < len(want[0]) < len(chunk_ref.corners(p))           # the threshold drops some corners and keeps some
    assert_chunks_equal(chunks_on_device(dropin, p, thresh), want)
    # the counts of every inner and widened box, one launch
    cs, mg = np.asarray(chunk_ref.CHUNK_SIZE), np.asarray(chunk_ref.MARGIN)
    corners = chunk_ref.corners(p)
    if corners:
        boxes = np.array([np.hstack([c, c + cs]) for c in corners] + [np.hstack([c - mg, c + cs + mg]) for c in corners])
        counts = ops.box_count(dev(p), boxes)
        want_counts = [int(chunk_ref.members(p, b[:2], b[2:]).sum()) for b in boxes]
        assert counts.dtype == torch.int64 and host(counts).tolist() == want_counts


def test_chunks_from_numpy_input_and_without_bbox(dropin, g17):
    cu = dropin("dropin.mvpnet.utils.chunk_util")
    p = g17["points"]
    thresh = int(g17["thresholds"][0])
    got = cu.scene2chunks_legacy(p, chunk_ref.CHUNK_SIZE, chunk_ref.STRIDE, thresh=thresh, margin=chunk_ref.MARGIN)
    want = chunk_ref.scene2chunks(p, thresh=thresh)[0]
    assert isinstance(got, list) and len(got) == len(want)
    assert all(isinstance(a, np.ndarray) and a.dtype == np.int64 and np.array_equal(a, b) for a, b in zip(got, want))
    with pytest.raises(TypeError):
        cu.scene2chunks_legacy(p.astype(np.float64), chunk_ref.CHUNK_SIZE, chunk_ref.STRIDE)


def test_one_point_reaches_the_kernels(ops):
    # scene2chunks_legacy has no corner for a single point, so the kernels see N = 1 only through the ops
    p = np.array([[0.25, -1.5, 3.0]], np.float32)
    boxes = np.array([[0.25, -1.5, 0.25, -1.5],          # the point is all four edges of this box
                      [0.0, -2.0, 1.0, -1.0],
                      [0.2500001, -2.0, 1.0, -1.0],      # just outside in x
                      [0.0, -2.0, 1.0, -1.5000001]])     # just outside in y
    counts = host(ops.box_count(dev(p), boxes))
    assert counts.tolist() == [1, 1, 0, 0]
    offsets, idx, zmin, zmax = ops.box_select(dev(p), boxes, counts)
    assert host(offsets).tolist() == [0, 1, 2, 2, 2] and host(idx).tolist() == [0, 0]
    assert host(zmin).tolist() == [3.0, 3.0, np.inf, np.inf] and host(zmax).tolist() == [3.0, 3.0, -np.inf, -np.inf]


def test_confusion_over_more_pairs_than_one_grid_pass(ops):
    # 300 000 pairs: more than 1 024 workgroups x 256 lanes, so the grid strides
    C, n = 7, 300000
    rng = np.random.default_rng(12)
    pred, truth = rng.integers(-1, C + 2, size=n), rng.integers(-2, C + 1, size=n)
    truth[::11] = -100
    got = ops.chunk_confusion(dev(pred), dev(truth), C)
    assert got.dtype == torch.int64 and np.array_equal(host(got), chunk_ref.confusion(truth, pred, C))


def test_more_boxes_than_one_lds_group(ops):
    # 300 boxes: the count kernel takes its boxes 256 at a time, the select kernels 64 at a time
    p = chunk_ref.random_scene(10, 2500)
    rng = np.random.default_rng(11)
    lo = rng.random((300, 2)) * (2.0, 1.5) + (0.1, 0.3)
    boxes = np.hstack([lo, lo + rng.random((300, 2))])
    boxes[7] = (9.0, 9.0, 9.5, 9.5)                                    # an empty box
    want = [np.nonzero(chunk_ref.members(p, b[:2], b[2:]))[0] for b in boxes]
    counts = host(ops.box_count(dev(p), boxes))
    assert counts.tolist() == [len(w) for w in want]
    offsets, idx, zmin, zmax = ops.box_select(dev(p), boxes, counts)
    assert host(offsets).tolist() == np.concatenate([[0], np.cumsum(counts)]).tolist()
    assert np.array_equal(host(idx), np.concatenate(want))
    zl, zh = host(zmin), host(zmax)
    for b, w in enumerate(want):
        if len(w):
            assert zl[b] == p[w, 2].min() and zh[b] == p[w, 2].max()
    assert zl[7] == np.inf and zh[7] == -np.inf


# -------------------------------------------------------------------------------------------------------------- vote

VOTE_SIZES = [1, 63, 64, 65, 1000, 1000, 65, 64, 63, 1, 1000, 129]     # 12 chunks, in this order
VOTE_PAD = [0, 1, 0, 63, 24, 0, 0, 64, 0, 7, 1048, 0]                  # ld - n per chunk
N_VOTE = 1301                                                          # rows 1200.. are never visited


def vote_case(C, seed):
    rng = np.random.default_rng(seed)
    chunks = []
    for n, pad in zip(VOTE_SIZES, VOTE_PAD):
        table = chunk_ref.table_logits(int(rng.integers(1 << 30)), C, [n], ld_extra=pad)[0]
        ind = rng.choice(1200, size=n, replace=False).astype(np.int64)
        if n != 129:
            ind = np.sort(ind)                                         # np.nonzero order; one chunk in any order
        chunks.append((table, ind))
    labels = rng.integers(0, C, size=N_VOTE).astype(np.int64)
    labels[rng.random(N_VOTE) < 0.05] = -100
    labels[rng.random(N_VOTE) < 0.03] = -1
    labels[rng.random(N_VOTE) < 0.03] = C
    labels[rng.random(N_VOTE) < 0.02] = C + 3
    return chunks, labels


@pytest.mark.parametrize("C", [20, 5])
def test_vote_is_bit_equal_to_the_restatement(ops, dropin, C):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    ev_mod = dropin("dropin.mvpnet.evaluate_3d")
    chunks, labels = vote_case(C, 40 + C)
    sums, visits, mean, pred = chunk_ref.vote_scene(N_VOTE, C, chunks)
    assert (visits == 0).sum() >= 101 and visits.max() >= 3
    # exact ties inside visited rows: the first maximum must win
    top = mean.max(axis=1, keepdims=True)
    assert ((mean == top).sum(axis=1)[visits > 0] > 1).any()

    voter = tm.WholeSceneVoter(N_VOTE, C, "cuda")
    for table, ind in chunks:
        voter.add(dev(table), dev(ind))
    assert util.bits_equal(host(voter.logit_sum), sums) and np.array_equal(host(voter.num_pred), visits)
    ev = ev_mod.Evaluator(["c%d" % i for i in range(C)])
    lab = dev(labels)
    got_pred, got_mean = voter.finish(lab, ev)
    assert got_pred.dtype == torch.int64 and np.array_equal(host(got_pred), pred)
    assert util.bits_equal(host(got_mean), mean)
    assert (host(got_pred)[visits == 0] == C).all()
    want = chunk_ref.evaluator_update(np.zeros((C, C)), pred, labels, C)
    assert ev.confusion_matrix.dtype == np.float64 and np.array_equal(ev.confusion_matrix, want) and want.sum() > 0
    assert np.array_equal(host(lab), labels)                            # tensors are not rewritten
    assert util.bits_equal(np.asarray(ev.class_iou), np.asarray(chunk_ref.class_iou(want)))
    assert ev.overall_acc == chunk_ref.overall_acc(want)
    # Evaluator.update on tensors counts the same pairs; all-negative truth leaves it as it is
    ev2 = ev_mod.Evaluator(["c%d" % i for i in range(C)])
    ev2.update(got_pred, lab)
    assert np.array_equal(ev2.confusion_matrix, want)
    ev2.update(got_pred, dev(np.where(labels >= 0, -100, labels)))
    assert np.array_equal(ev2.confusion_matrix, want)
    # the division by max(visits, 1) without the in-place overwrite, and the confusion accumulating into a given matrix
    s2, c2 = dev(sums), dev(visits)
    conf = torch.ones((C, C), dtype=torch.int64, device="cuda")
    p3, m3, conf = ops.chunk_vote_finish(s2, c2, labels=lab, confusion=conf)
    assert util.bits_equal(host(s2), sums) and util.bits_equal(host(m3), mean) and np.array_equal(host(p3), pred)
    assert np.array_equal(host(conf), want.astype(np.int64) + 1)


def test_vote_reference_outputs_of_the_fixture(dropin, g17):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    ev_mod = dropin("dropin.mvpnet.evaluate_3d")
    p = g17["points"]
    indices, _ = chunks_on_device(dropin, p, int(g17["thresholds"][0]))
    tables = chunk_ref.table_logits(int(g17["logit_seed"]), C20, [len(i) for i in indices])
    voter = tm.WholeSceneVoter(len(p), C20, "cuda")
    for table, ind in zip(tables, indices):
        voter.add(dev(table), ind)
    ev = ev_mod.Evaluator(["c%d" % i for i in range(C20)])
    pred, mean = voter.finish(g17["labels"], ev)
    assert np.array_equal(host(voter.num_pred), g17["t0/visits"]) and np.array_equal(host(pred), g17["t0/pred"])
    assert util.bits_equal(host(mean), g17["t0/mean"]) and np.array_equal(ev.confusion_matrix, g17["t0/confusion"])
    assert ev.overall_iou == float(g17["t0/overall_iou"])


def test_vote_index_outside_the_scene_writes_nothing(ops):
    C, N = 5, 100
    table = chunk_ref.table_logits(3, C, [70])[0]
    ind = np.arange(10, 80).astype(np.int64)
    ind[[0, 33, 69]] = (-1, N, 1 << 40)
    sums, counts = torch.zeros((N, C), device="cuda"), torch.zeros((N,), dtype=torch.int32, device="cuda")
    ops.chunk_vote_add(sums, counts, dev(table), dev(ind))
    ok = (ind >= 0) & (ind < N)
    want = chunk_ref.vote_scene(N, C, [(table[:, ok], ind[ok])])
    assert util.bits_equal(host(sums), want[0]) and np.array_equal(host(counts), want[1])
    with pytest.raises(RuntimeError, match="indices"):
        ops.chunk_vote_add(sums, counts, dev(table[:, :10]), dev(ind))


def test_evaluator_with_a_label_table_on_tensors(dropin):
    ev_mod = dropin("dropin.mvpnet.evaluate_3d")
    ev = ev_mod.Evaluator(["a", "b", "c"], labels=[4, 9, 2])
    ev.update(dev(np.array([4, 9, 2, 2, 7, 4])), dev(np.array([4, 4, 2, 9, 4, 5])))
    assert ev.confusion_matrix.tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 1]]


# ------------------------------------------------------------------------------------------ end to end, table logits

class TableModel(torch.nn.Module):
    """Stands for the network: returns the next pre-generated logit table and keeps what it was given."""

    def __init__(self, tables):
        super().__init__()
        self.tables, self.seen, self.modes = list(tables), [], []

    def forward(self, batch):
        self.modes.append((self.training, torch.is_grad_enabled()))
        self.seen.append({k: v for k, v in batch.items()})
        return {"seg_logit": self.tables[len(self.seen) - 1].unsqueeze(0)}


def test_predict_whole_scene_with_table_logits(dropin, g17):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    ev_mod = dropin("dropin.mvpnet.evaluate_3d")
    p, labels = g17["points"], g17["labels"]
    indices, _ = chunks_on_device(dropin, p, int(g17["thresholds"][2]))
    sizes = sorted(len(i) for i in indices)
    min_nb_pts = sizes[0] + 37                                          # exactly one chunk is below it
    assert sizes[0] < min_nb_pts <= sizes[1]
    rng = np.random.default_rng(5)
    pts = dev(p)
    inputs, tables = [], []
    for ind in indices:
        nc = len(ind)
        inputs.append({"points": pts[ind].t().contiguous(), "chunk_ind": ind, "images": torch.zeros(1, 3, 2, 2, device="cuda"),
                       "image_xyz": torch.zeros(1, 2, 2, 3, device="cuda"),
                       "knn_indices": dev(rng.integers(0, 4, size=(nc, 3)).astype(np.int64))})
        tables.append(chunk_ref.table_logits(int(rng.integers(1 << 30)), C20, [max(nc, min_nb_pts)])[0])
    model = TableModel([dev(t) for t in tables]).train()
    ev = ev_mod.Evaluator(["c%d" % i for i in range(C20)])
    np.random.seed(1234)
    pred, mean = tm.predict_whole_scene(model, pts, inputs, min_nb_pts=min_nb_pts, seg_label=dev(labels), evaluator=ev)

    np.random.seed(1234)
    padded = 0
    for d, seen in zip(inputs, model.seen):
        nc = len(d["chunk_ind"])
        choice = chunk_ref.pad_choice(nc, min_nb_pts) if nc < min_nb_pts else np.arange(nc)
        padded += nc < min_nb_pts
        assert seen["points"].shape == (1, 3, len(choice)) and seen["knn_indices"].shape == (1, len(choice), 3)
        assert np.array_equal(host(seen["points"][0]), host(d["points"])[:, choice])
        assert np.array_equal(host(seen["knn_indices"][0]), host(d["knn_indices"])[choice])
    assert padded == 1 and all(m == (False, False) for m in model.modes) and model.training
    want = chunk_ref.vote_scene(len(p), C20, [(t, host(i)) for t, i in zip(tables, indices)])
    assert np.array_equal(host(pred), want[3]) and util.bits_equal(host(mean), want[2])
    m = chunk_ref.evaluator_update(np.zeros((C20, C20)), want[3], labels, C20)
    assert np.array_equal(ev.confusion_matrix, m)
    assert util.bits_equal(np.asarray(ev.class_iou), np.asarray(chunk_ref.class_iou(m)))
    assert ev.overall_acc == chunk_ref.overall_acc(m) and ev.overall_iou == np.nanmean(chunk_ref.class_iou(m))


def test_a_scene_without_chunks_predicts_the_extra_label_everywhere(dropin):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    ev_mod = dropin("dropin.mvpnet.evaluate_3d")
    p = chunk_ref.small_scene(3, 777, 1.0)
    indices, boxes = chunks_on_device(dropin, p, 1)
    assert indices == [] and boxes == []
    ev = ev_mod.Evaluator(["a", "b", "c", "d"])
    labels = dev(np.arange(777) % 4)
    pred, mean = tm.predict_whole_scene(torch.nn.Identity(), dev(p), [], seg_label=labels, evaluator=ev)
    assert pred.shape == (777,) and (host(pred) == 4).all() and mean.shape == (777, 4) and not host(mean).any()
    assert not ev.confusion_matrix.any()
    with pytest.raises(ValueError):
        tm.predict_whole_scene(torch.nn.Identity(), dev(p), [])


# --------------------------------------------------------------------------------------- end to end, the real network

class StandIn2D(torch.nn.Module):
    """Stands for the 2D encoder: {'image': (n,3,h,w)} -> {'feature': (n,c,h,w)}."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def synthetic_frames(points, nf=5, h=12, w=16, nb=400, seed=21):
    """Depth frames looking along +z from below the scene, each shifted in xy: pixels land all over the scene's xy
    extent. One frame has no valid depth at all, another has holes."""
    rng = np.random.default_rng(seed)
    cam = np.array([[6.0, 0, w / 2], [0, 6.0, h / 2], [0, 0, 1]], np.float32)
    depth = rng.integers(900, 2100, size=(nf, h, w)).astype(np.int16)
    depth[1] = 0
    depth[2][rng.random((h, w)) < 0.3] = 0
    poses = np.tile(np.eye(4, dtype=np.float32), (nf, 1, 1))
    centre = (points.max(0) + points.min(0)) / 2
    for f in range(nf):
        poses[f, :3, 3] = (centre[0] + 0.4 * (f - 2), centre[1] - 0.3 * (f - 2), -1.0)
    return {"depth": dev(depth), "images": dev(rng.standard_normal((nf, h, w, 3)).astype(np.float32)), "poses": dev(poses),
            "cam_matrix": cam, "base_point_ind": dev(np.sort(rng.choice(len(points), nb, replace=False)).astype(np.int64)),
            "pointwise_rgbd_overlap": dev(rng.random((nb, nf)) < 0.3)}


def select_frames_np(overlap, n):
    overlap, out = overlap.copy(), []
    for _ in range(n):
        f = int(overlap.sum(0).argmax())
        out.append(f)
        overlap[overlap[:, f]] = False
    return out


def test_predict_whole_scene_with_the_real_network(ops, dropin, g17):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    torch.manual_seed(3)
    c, n_cls, k, nv = 8, 5, 3, 2
    net_3d = PN2SSG(8, n_cls, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                    fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    p = g17["points"]
    pts = dev(p)
    frames = synthetic_frames(p)
    indices, boxes = chunks_on_device(dropin, p, int(g17["thresholds"][0]))
    inputs = [tm.chunk_rgbd_inputs(pts, ind, box, frames, nv, k=k) for ind, box in zip(indices, boxes)]

    # one chunk's frame choice, pixel mask and k-NN against NumPy in float64
    ci = 2
    d, box, ind = inputs[ci], boxes[ci], host(indices[ci])
    in_chunk = np.zeros(len(p), bool)
    in_chunk[ind] = True
    bpi = host(frames["base_point_ind"])
    sel = select_frames_np(host(frames["pointwise_rgbd_overlap"])[in_chunk[bpi]], nv)
    assert np.array_equal(host(d["images"]), np.moveaxis(host(frames["images"])[sel], -1, 1))
    xyz, valid = ops.unproject_depth(frames["depth"][sel], frames["cam_matrix"], frames["poses"][sel])
    xyz, valid = host(xyz), host(valid)
    assert xyz.dtype == np.float64 and util.bits_equal(host(d["image_xyz"]), xyz.astype(np.float32))
    mask = valid & (xyz[..., 0] > box[0] - 0.1) & (xyz[..., 0] < box[3] + 0.1) & (xyz[..., 1] > box[1] - 0.1) & \
        (xyz[..., 1] < box[4] + 0.1)
    assert np.array_equal(host(d["image_mask"]), mask) and k <= mask.sum() < valid.sum()
    keys, flat = xyz.reshape(-1, 3)[mask.reshape(-1)], np.nonzero(mask.reshape(-1))[0]
    q = p[ind].astype(np.float64)
    diff = q[:, None, :] - keys[None, :, :]
    d2 = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
    want_knn = flat[np.argsort(d2, axis=1, kind="stable")[:, :k]]
    assert d["knn_indices"].dtype == torch.int64 and np.array_equal(host(d["knn_indices"]), want_knn)
    assert np.array_equal(host(d["points"]), p[ind].T) and d["images"].shape == (nv, 3, 12, 16)

    pred, mean = tm.predict_whole_scene(net, pts, inputs, min_nb_pts=64)
    # the same chunks forwarded one by one and accumulated with torch
    sums = torch.zeros((len(p), n_cls), device="cuda")
    visits = torch.zeros((len(p),), dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for d in inputs:
            batch = {key: d[key].unsqueeze(0) for key in ("points", "images", "image_xyz", "knn_indices")}
            logit = net(batch)["seg_logit"][0]
            assert logit.shape == (n_cls, len(d["chunk_ind"]))
            sums.index_add_(0, d["chunk_ind"], logit.t().contiguous())
            visits.index_add_(0, d["chunk_ind"], torch.ones_like(d["chunk_ind"], dtype=torch.int32))
    sums, visits = host(sums), host(visits)
    want_mean = sums / np.maximum(visits, 1)[:, None].astype(np.float32)
    want_pred = np.argmax(want_mean, axis=1)
    want_pred[visits == 0] = n_cls
    assert np.array_equal(visits, g17["t0/visits"]) and (visits == 0).any()
    assert util.bits_equal(host(mean), want_mean) and np.array_equal(host(pred), want_pred)
    ops.pn2_check_indices()                                 # no interpolation met an index outside its key set


def test_chunk_rgbd_inputs_needs_k_valid_pixels(dropin, g17):
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    p = g17["points"]
    frames = synthetic_frames(p)
    frames["depth"] = torch.zeros_like(frames["depth"])
    indices, boxes = chunks_on_device(dropin, p, int(g17["thresholds"][0]))
    with pytest.raises(ValueError, match="n_neighbors"):
        tm.chunk_rgbd_inputs(dev(p), indices[0], boxes[0], frames, 2, k=3)
