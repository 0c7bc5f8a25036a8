"""GPU: the ragged point ops (mvk_fps_ragged, mvk_pn2_ball_query_ragged) against tests/pn2_ragged_ref.py and against
the plain ops on each cloud alone (exact), PN2SSG / MVPNet3D with data_batch['lengths'] against their one-cloud
forwards, and predict_whole_scene_grouped(chunks_per_forward=G) against G = 1 (predict_whole_scene itself)."""
import copy

import numpy as np
import pytest
import torch

import chunk_ref
import pn2_ragged_ref
import pn2_ref
import util

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def fill_padding(block, lengths, how, rng):
    """Rows at or beyond n_b of a padded (B,N,D) block: NaN, or copies of the cloud's row 0 (duplicates change nothing
    in FPS, but would be ball-query hits), or other points of the same box (which would be picked if they were read)."""
    for b, n in enumerate(lengths):
        if how == "nan":
            block[b, n:] = np.nan
        elif how == "row0":
            block[b, n:] = block[b, 0]
        else:
            block[b, n:] = rng.random(block[b, n:].shape) * 3 - 1
    return block


# ------------------------------------------------------------------------------------------------ farthest point sampling

# padded N, M, lengths: M, M + 1, N and one between, then the power-of-two edges that fit. One batch per path: 1, 2, 4,
# 8 and 16 points per lane (float64 leaves the registers above 8 192), then the workspace kernel per dtype.
EDGES = [511, 512, 513]
FPS_PATHS = {
    64: (8, [8, 9, 64, 33, 15, 16, 17]),
    1000: (24, [24, 25, 1000, 600] + EDGES),
    1025: (129, [129, 130, 1025, 700] + EDGES + [1023]),
    4100: (24, [24, 25, 4100, 2000] + EDGES + [1023]),
    16384: (16, [16, 17, 16384, 9000] + EDGES + [1023]),
    "workspace": (16, None),
}


def fps_path(n_pad, dtype):
    if n_pad == "workspace":
        n_pad = 16385 if dtype == np.float32 else 8193
        return n_pad, 16, [16, 17, n_pad, 5000] + EDGES + [1023]
    m, lengths = FPS_PATHS[n_pad]
    return n_pad, m, lengths


def check_fps(ops, pts, lengths, m, plain=True):
    """The ragged call against the helper and, cloud by cloud, against the plain op on the slice."""
    got = host(ops.fps(dev(pts), m, lengths=dev(np.asarray(lengths, np.int64))))
    clean = np.where(np.isnan(pts), 0, pts)                             # the helper slices; NaN rows never reach it
    want = pn2_ragged_ref.fps(clean, lengths, m)
    assert got.dtype == np.int64 and np.array_equal(got, want), [b for b in range(len(got)) if not np.array_equal(got[b], want[b])]
    if plain:
        for b, n in enumerate(lengths):
            alone = host(ops.fps(dev(pts[b:b + 1, :n]), min(m, n)))[0]
            assert np.array_equal(got[b, :len(alone)], alone), (b, n)
    return got


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("fill", ["nan", "row0"])
@pytest.mark.parametrize("path", list(FPS_PATHS))
def test_fps_with_lengths_on_random_clouds(ops, path, fill, d, dtype):
    n_pad, m, lengths = fps_path(path, dtype)
    rng = np.random.default_rng(n_pad + d)
    pts = fill_padding(rng.random((len(lengths), n_pad, d)).astype(dtype), lengths, fill, rng)
    check_fps(ops, pts, lengths, m)


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_with_lengths_breaks_ties_like_each_cloud_alone(ops, dtype):
    # lattice clouds: every round has ties, and 125 sites at most, so m = 140 runs out and repeats
    for n_pad, m, lengths in ((1000, 140, [140, 141, 1000, 300] + EDGES), (64, 16, [16, 17, 64, 33]),
                              (130, 40, [40, 41, 130, 70]), (1025, 64, [64, 65, 1025, 1023, 512, 513])):
        rng = np.random.default_rng(m)
        pts = np.stack([pn2_ref.lattice_cloud(n_pad, 50 + i) for i in range(len(lengths))]).astype(dtype)
        got = check_fps(ops, fill_padding(pts, lengths, "other", rng), lengths, m)
        for b, n in enumerate(lengths):
            assert np.array_equal(got[b], pn2_ref.fps_literal(pts[b, :n], m)), (n_pad, n)     # the reference's own schedule
        if m == 140:
            assert (got[:, -1] == got[:, -2]).all()


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_cloud_smaller_than_the_sample_repeats_its_last_pick(ops, dtype):
    rng = np.random.default_rng(8)
    lengths, m = [5, 64, 1, 20], 20
    pts = fill_padding(rng.random((4, 64, 3)).astype(dtype), lengths, "nan", rng)
    got = check_fps(ops, pts, lengths, m)
    assert len(set(got[0, :5].tolist())) == 5 and (got[0, 5:] == got[0, 4]).all() and (got[2] == 0).all()
    # a count outside [1, N] is clamped into it
    clamped = host(ops.fps(dev(pts), m, lengths=dev(np.array([5, 64 + 9, 0, 20], np.int64))))
    assert np.array_equal(clamped, got)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("path", list(FPS_PATHS))
def test_fps_with_full_lengths_is_the_plain_call(ops, path, dtype):
    n_pad, m, _ = fps_path(path, dtype)
    pts = dev(np.random.default_rng(3).random((3, n_pad, 3)).astype(dtype))
    full = torch.full((3,), n_pad, dtype=torch.int64, device="cuda")
    assert torch.equal(ops.fps(pts, m, lengths=full), ops.fps(pts, m))


def test_lengths_must_live_with_the_points(ops):
    pts = dev(np.zeros((2, 8, 3), np.float32))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fps(pts, 2, lengths=torch.tensor([8, 5]))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.pn2_ball_query(pts, pts, 0.1, 2, key_lengths=torch.tensor([8, 5]))
    with pytest.raises(RuntimeError, match="int64"):
        ops.fps(pts, 2, lengths=torch.tensor([8, 5], dtype=torch.int32).cuda())
    with pytest.raises(RuntimeError, match="shape"):
        ops.pn2_ball_query(pts, pts, 0.1, 2, key_lengths=torch.tensor([8]).cuda())
    with pytest.raises(RuntimeError, match="centroids"):                # the host entry still requires 1 <= M <= N
        ops.fps(pts, 9, lengths=torch.tensor([8, 5]).cuda())


# ------------------------------------------------------------------------------------------------ ball query

BQ_LENGTHS = lambda n2: [1, 63, 64, 65, n2]
N1 = 20


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("k", [1, 32, 70])
@pytest.mark.parametrize("n2", [130, 1000])
def test_ball_query_with_key_lengths(ops, n2, k, dtype):
    lengths = BQ_LENGTHS(n2)
    rng = np.random.default_rng(n2 + k)
    key = rng.random((len(lengths), n2, 3)).astype(dtype)
    q = key[:, rng.permutation(n2)[:N1]].copy()                         # queries at keys, valid ones or not
    q[:, 3] = 1000.0                                                    # no key near it: a row of -1
    for b, n in enumerate(lengths):                                     # the padding repeats the queries: hits, if read
        key[b, n:] = q[b, np.arange(n2 - n) % N1]
    radius = 0.25
    want_i, want_d = pn2_ragged_ref.ball_query(q, key, lengths, radius, k)
    assert (want_i[:, 3] == -1).all() and all(want_i[b].max() < n for b, n in enumerate(lengths))
    if k > 1:                                                           # rows padded with the first hit ...
        assert (want_d == -1).any() and (want_d[-1] >= 0).any()
    if n2 == 1000 and k < 70:                                           # ... and rows cut at K
        assert (want_d[-1, :, -1] >= 0).any()
    kl = dev(np.asarray(lengths, np.int64))
    got_i, got_d = ops.pn2_ball_query(dev(q), dev(key), radius, k, with_distance=True, key_lengths=kl)
    assert got_i.dtype == torch.int64 and got_d.dtype == dev(q).dtype
    assert np.array_equal(host(got_i), want_i) and util.bits_equal(host(got_d), want_d)
    assert np.array_equal(host(ops.pn2_ball_query(dev(q), dev(key), radius, k, key_lengths=kl)), want_i)
    for b, n in enumerate(lengths):                                     # and the plain op on the slice
        alone_i, alone_d = ops.pn2_ball_query(dev(q[b:b + 1]), dev(key[b:b + 1, :n]), radius, k, with_distance=True)
        assert torch.equal(alone_i[0], got_i[b]) and util.bits_equal(host(alone_d[0]), host(got_d[b]))
    if n2 == 130 and k == 32:                                           # the drop-in's wrappers, both layouts
        import mvkpconv
        bq = mvkpconv.sub("dropin.mvpnet.ops.ball_query")
        assert np.array_equal(host(bq.ball_query(dev(q), dev(key), radius, k, transpose=False, key_lengths=kl)), want_i)
        ti, td = bq.ball_query_distance(dev(q).transpose(1, 2), dev(key).transpose(1, 2), radius, k, key_lengths=kl)
        assert np.array_equal(host(ti), want_i) and util.bits_equal(host(td), want_d)
        full = torch.full((len(lengths),), n2, dtype=torch.int64, device="cuda")
        assert torch.equal(ops.pn2_ball_query(dev(q), dev(key), radius, k, key_lengths=full),
                           ops.pn2_ball_query(dev(q), dev(key), radius, k))


# ------------------------------------------------------------------------------------------------ the network

def ragged_pn2_case(dropin, golden):
    """The g16 PointNet++ (fixture weights), three clouds of 256, 219 and 64 = num_centroids[0] points in one padded
    batch whose padding would change centroids and neighbours if it were read."""
    import test_pn2_frozen_gpu as tf
    net, batch = tf.g16_net(dropin, golden)
    rng = np.random.default_rng(161)
    n = batch["points"].shape[2]
    lengths = [n, n - 37, net.sa_modules[0].num_centroids]
    points = np.concatenate([host(batch["points"]), tf.dyadic(rng, (1, 3, n))])
    feature = np.concatenate([host(batch["feature"]), rng.standard_normal((1, 4, n)).astype(np.float32)])
    singles = [{"points": dev(points[b:b + 1, :, :nb]), "feature": dev(feature[b:b + 1, :, :nb])}
               for b, nb in enumerate(lengths)]
    points[1, :, lengths[1]:] = points[1, :, :1]                        # copies of the cloud's first point
    points[2, :, lengths[2]:] = tf.dyadic(rng, (3, n - lengths[2]))     # other points of the same box
    for b, nb in enumerate(lengths):
        feature[b, :, nb:] = 1e6
    padded = {"points": dev(points), "feature": dev(feature), "lengths": dev(np.asarray(lengths, np.int64))}
    return net, padded, singles, lengths


def hooked_forward(net, batch):
    """seg_logit and every SetAbstraction's (new_xyz, new_feature)."""
    seen = []
    hooks = [sa.register_forward_hook(lambda m, i, o: seen.append(o)) for sa in net.sa_modules]
    try:
        with torch.no_grad():
            out = net(batch)["seg_logit"]
    finally:
        for h in hooks:
            h.remove()
    return out, seen


def referee_per_cloud(label, net, padded_out, singles, lengths, single_outs):
    import test_pn2_frozen_gpu as tf
    failures, equal = [], []
    for b, nb in enumerate(lengths):
        got = host(padded_out[b:b + 1, :, :nb])
        util.referee_check("%s, cloud %d of %d points" % (label, b, nb), got, host(single_outs[b]),
                           tf.float64_forward(net, singles[b]), failures=failures)
        equal.append(util.bits_equal(got, host(single_outs[b])))
    print("%s: logits bit-equal to the one-cloud forward per cloud: %s" % (label, equal))
    assert not failures, "\n".join(failures)


@pytest.mark.parametrize("frozen", [True, False], ids=["frozen", "unfrozen"])
def test_pn2ssg_with_lengths_is_each_cloud_alone(ops, dropin, golden, frozen):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    net, padded, singles, lengths = ragged_pn2_case(dropin, golden)
    if frozen:
        modules.freeze_inference(net)
        assert all(sa._frozen is not None for sa in net.sa_modules)
    out, levels = hooked_forward(net, padded)
    assert out.shape == (3, 5, 256) and [lv[0].shape[2] for lv in levels] == [64, 16]
    single_outs = []
    for b, one in enumerate(singles):
        one_out, one_levels = hooked_forward(net, one)
        single_outs.append(one_out)
        for lv, ((xyz, feat), (one_xyz, one_feat)) in enumerate(zip(levels, one_levels)):
            assert torch.equal(xyz[b:b + 1], one_xyz), (b, lv)          # the same centroids, in the same order
            if frozen:      # FPS, a gather, the ball query and the fused launch are all row-wise: the same bits
                assert util.bits_equal(host(feat[b:b + 1]), host(one_feat)), (b, lv)
    referee_per_cloud("PN2SSG with lengths, " + ("frozen" if frozen else "unfrozen eval"), net, out, singles, lengths,
                      single_outs)
    ops.pn2_check_indices()


def test_pn2ssg_with_lengths_refuses_training_mode(dropin, golden):
    net, padded, _, _ = ragged_pn2_case(dropin, golden)
    with pytest.raises(RuntimeError, match="inference"):
        net.train()(padded)
    with torch.no_grad():
        net.eval()(padded)                                              # and eval mode takes it again


def test_mvpnet3d_with_lengths_within_the_referee_of_one_by_one(ops, dropin):
    import test_chunk_gpu as tc
    import test_pn2_frozen_gpu as tf
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    torch.manual_seed(3)
    b, nv, h, w, c, n_pts, k = 3, 2, 6, 8, 8, 128, 3
    net_3d = pn2ssg.PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(tc.StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    tf.perturb_batchnorm(net, np.random.default_rng(18))
    rng = np.random.default_rng(19)
    lengths = [n_pts, n_pts - 37, 32]
    batch = {"images": torch.randn(b, nv, 3, h, w).cuda(), "image_xyz": torch.rand(b, nv, h, w, 3).cuda(),
             "knn_indices": torch.randint(0, nv * h * w, (b, n_pts, k)).cuda(), "points": dev(tf.dyadic(rng, (b, 3, n_pts)))}
    singles = [{key: (v[i:i + 1, :, :nb] if key == "points" else v[i:i + 1, :nb] if key == "knn_indices" else v[i:i + 1])
                for key, v in batch.items()} for i, nb in enumerate(lengths)]
    singles = [{key: v.clone() for key, v in one.items()} for one in singles]
    for i, nb in enumerate(lengths):                                    # the padding of collate_chunks: zeros
        batch["points"][i, :, nb:] = 0
        batch["knn_indices"][i, nb:] = 0
    batch["lengths"] = dev(np.asarray(lengths, np.int64))
    for frozen in (False, True):
        if frozen:
            pn2ssg.freeze_inference(net)
            assert net_3d.sa_modules[0]._frozen is not None
        with torch.no_grad():
            out = net(batch)["seg_logit"]
            single_outs = [net(one)["seg_logit"] for one in singles]
        referee_per_cloud("MVPNet3D with lengths, " + ("frozen" if frozen else "unfrozen eval"), net, out, singles,
                          lengths, single_outs)
    ops.pn2_check_indices()


# ------------------------------------------------------------------------------------------------ the loop

C20 = 20


class GroupTableModel(torch.nn.Module):
    """Stands for a network that takes 'lengths': returns the next G pre-generated logit tables as [G, C, n_max], NaN
    behind each chunk's own columns (they must not vote), and keeps what it was given."""

    def __init__(self, tables):
        super().__init__()
        self.tables, self.seen, self.modes, self.at = list(tables), [], [], 0

    def forward(self, batch):
        self.modes.append((self.training, torch.is_grad_enabled()))
        self.seen.append(dict(batch))
        if "lengths" not in batch:                                      # chunks_per_forward = 1: today's call
            self.at += 1
            return {"seg_logit": self.tables[self.at - 1].unsqueeze(0)}
        g, n_max = batch["points"].shape[0], batch["points"].shape[2]
        out = torch.full((g, self.tables[0].shape[0], n_max), float("nan"), device="cuda")
        for i in range(g):
            t = self.tables[self.at + i]
            out[i, :, :t.shape[1]] = t
        self.at += g
        return {"seg_logit": out}


@pytest.fixture(scope="module")
def table_scene(dropin, golden):
    """The g17 scene cut into 8 chunks with exactly one below min_nb_pts, table logits, and the G = 1 result."""
    import test_chunk_gpu as tc
    tm = dropin("dropin.mvpnet.whole_scene_grouped")
    g17 = golden("g17_mvpnet_chunks")
    p, labels = g17["points"], g17["labels"]
    indices, _ = tc.chunks_on_device(dropin, p, int(g17["thresholds"][2]))
    sizes = sorted(len(i) for i in indices)
    min_nb_pts = sizes[0] + 37
    assert len(indices) == 8 and sizes[0] < min_nb_pts <= sizes[1]
    rng = np.random.default_rng(5)
    pts = dev(p)
    inputs, tables = [], []
    for ind in indices:
        nc = len(ind)
        inputs.append({"points": pts[ind].t().contiguous(), "chunk_ind": ind, "images": torch.zeros(1, 3, 2, 2, device="cuda"),
                       "image_xyz": torch.zeros(1, 2, 2, 3, device="cuda"),
                       "knn_indices": dev(rng.integers(1, 4, size=(nc, 3)).astype(np.int64))})
        tables.append(dev(chunk_ref.table_logits(int(rng.integers(1 << 30)), C20, [max(nc, min_nb_pts)])[0]))
    return dict(tm=tm, pts=pts, labels=dev(labels), inputs=inputs, tables=tables, min_nb_pts=min_nb_pts,
                base=run_table_scene(dropin, tm, pts, dev(labels), inputs, tables, min_nb_pts, 1))


def run_table_scene(dropin, tm, pts, labels, inputs, tables, min_nb_pts, g):
    ev = dropin("dropin.mvpnet.evaluate_3d").Evaluator(["c%d" % i for i in range(C20)])
    model = GroupTableModel(tables).train()
    voters = []

    class Spy(tm.WholeSceneVoter):
        def __init__(self, *a):
            super().__init__(*a)
            voters.append(self)

    one = dropin("dropin.mvpnet.test_mvpnet_3d")                        # G = 1 is its predict_whole_scene
    real, tm.WholeSceneVoter, one.WholeSceneVoter = tm.WholeSceneVoter, Spy, Spy
    try:
        np.random.seed(1234)
        pred, mean = tm.predict_whole_scene_grouped(model, pts, inputs, min_nb_pts=min_nb_pts, seg_label=labels,
                                                    evaluator=ev, chunks_per_forward=g)
    finally:
        tm.WholeSceneVoter = one.WholeSceneVoter = real
    assert len(voters) == 1 and model.training and all(m == (False, False) for m in model.modes)
    return dict(pred=host(pred), mean=host(mean), visits=host(voters[0].num_pred), confusion=ev.confusion_matrix.copy(),
                seen=model.seen)


@pytest.mark.parametrize("g", [2, 3, 32])
def test_chunks_per_forward_is_bit_equal_to_one_chunk_per_forward(dropin, table_scene, g):
    s = table_scene
    base = s["base"]
    assert len(base["seen"]) == 8 and all("lengths" not in seen for seen in base["seen"]) and base["visits"].max() >= 2
    got = run_table_scene(dropin, s["tm"], s["pts"], s["labels"], s["inputs"], s["tables"], s["min_nb_pts"], g)
    assert np.array_equal(got["pred"], base["pred"]) and util.bits_equal(got["mean"], base["mean"])
    assert np.array_equal(got["visits"], base["visits"]) and np.array_equal(got["confusion"], base["confusion"])
    assert got["confusion"].sum() > 0 and not np.isnan(got["mean"]).any()
    # what the model received: the chunks G at a time, each as the one-chunk loop passed it, zero-padded, with lengths
    assert [len(seen["lengths"]) for seen in got["seen"]] == [min(g, 8 - i) for i in range(0, 8, g)]
    at, padded = 0, 0
    for seen in got["seen"]:
        lengths = seen["lengths"]
        assert lengths.dtype == torch.int64 and lengths.is_cuda and set(seen) == set(base["seen"][0]) | {"lengths"}
        n_max = int(lengths.max())
        assert seen["points"].shape == (len(lengths), 3, n_max) and seen["knn_indices"].shape == (len(lengths), n_max, 3)
        for i, n in enumerate(lengths.tolist()):
            alone = base["seen"][at]
            padded += n > len(s["inputs"][at]["chunk_ind"])
            assert alone["points"].shape == (1, 3, n)
            assert torch.equal(seen["points"][i, :, :n], alone["points"][0]) and not seen["points"][i, :, n:].any()
            assert torch.equal(seen["knn_indices"][i, :n], alone["knn_indices"][0]) and not seen["knn_indices"][i, n:].any()
            assert torch.equal(seen["images"][i], alone["images"][0]) and torch.equal(seen["image_xyz"][i], alone["image_xyz"][0])
            at += 1
    assert at == 8 and padded == 1


def test_chunks_per_forward_with_the_real_frozen_network(ops, dropin, golden):
    import test_chunk_gpu as tc
    import test_pn2_frozen_gpu as tf
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    wg = dropin("dropin.mvpnet.whole_scene_grouped")
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    g17 = golden("g17_mvpnet_chunks")
    torch.manual_seed(3)
    c, n_cls, k, nv = 8, 5, 3, 2
    net_3d = pn2ssg.PN2SSG(8, n_cls, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(tc.StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    tf.perturb_batchnorm(net, np.random.default_rng(17))
    p = g17["points"]
    pts = dev(p)
    frames = tc.synthetic_frames(p)
    indices, boxes = tc.chunks_on_device(dropin, p, int(g17["thresholds"][2]))
    inputs = [tm.chunk_rgbd_inputs(pts, ind, box, frames, nv, k=k) for ind, box in zip(indices, boxes)]
    sizes = sorted(len(i) for i in indices)
    min_nb_pts = sizes[0] + 37                                          # one sparse chunk
    assert sizes[0] < min_nb_pts <= sizes[1] and len(set(sizes)) > 4

    # float64: the same chunks, padded with the same draws, one by one through the float64 network, summed in float64
    net64 = copy.deepcopy(net).double().eval()
    sums = torch.zeros((len(p), n_cls), dtype=torch.float64, device="cuda")
    visits = torch.zeros((len(p),), dtype=torch.float64, device="cuda")
    np.random.seed(99)
    with torch.no_grad():
        for d in inputs:
            nc = len(d["chunk_ind"])
            rows = dev(chunk_ref.pad_choice(nc, min_nb_pts) if nc < min_nb_pts else np.arange(nc))
            batch = {"points": d["points"][:, rows].double()[None], "knn_indices": d["knn_indices"][rows][None],
                     "images": d["images"].double()[None], "image_xyz": d["image_xyz"].double()[None]}
            logit = net64(batch)["seg_logit"][0, :, :nc]
            sums.index_add_(0, d["chunk_ind"], logit.t().contiguous())
            visits.index_add_(0, d["chunk_ind"], torch.ones_like(visits[:nc]))
    mean64 = host(sums / visits.clamp(min=1)[:, None])
    visited = host(visits) > 0

    pn2ssg.freeze_inference(net)
    assert net_3d.sa_modules[0]._frozen is not None

    def scene(g):
        np.random.seed(99)
        pred, mean = wg.predict_whole_scene_grouped(net, pts, inputs, min_nb_pts=min_nb_pts, chunks_per_forward=g)
        return host(pred), host(mean)

    def compare(label, pred, mean, ref_pred, ref_mean, cap=0.05):
        """Predictions where the top-two margin of ref_mean exceeds the largest logit difference of that point; the
        share of visited points left out must stay below the cap."""
        diff = np.abs(mean.astype(np.float64) - ref_mean).max(axis=1)
        top = np.sort(ref_mean.astype(np.float64), axis=1)
        decided = visited & (top[:, -1] - top[:, -2] > diff)
        left_out = 1.0 - decided[visited].mean()
        msg = "%s: largest logit difference %.3e, %.2f %% of the visited points left out (cap %.0f %%)" \
            % (label, diff[visited].max(), 100 * left_out, 100 * cap)
        print(msg)
        assert left_out <= cap, msg
        assert np.array_equal(pred[decided], ref_pred[decided]), msg
        assert np.array_equal(pred[~visited], ref_pred[~visited])

    pred1, mean1 = scene(1)
    pred64 = np.where(visited, mean64.argmax(axis=1), n_cls)
    compare("G = 1 against its float64 forward", pred1, mean1, pred64, mean64)
    failures = []
    for g in (2, 3, 32):
        pred, mean = scene(g)
        util.referee_check("whole scene, mean logits at G = %d (reference: G = 1)" % g, mean, mean1, mean64, failures=failures)
        compare("G = %d against G = 1" % g, pred, mean, pred1, mean1)
        print("G = %d: mean logits bit-equal to G = 1: %s" % (g, util.bits_equal(mean, mean1)))
    assert not failures, "\n".join(failures)
    ops.pn2_check_indices()
