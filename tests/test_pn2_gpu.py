"""GPU: the MVPNet baseline's point ops (csrc/pn2.hip) against the NumPy restatements (tests/pn2_ref.py) and the
outputs of the reference's own restatements (fixtures g15 / g16), the PointNet++ network of the drop-in against the
reference's classes (g16, float64 referee), and MVPNet3D against its wiring written out."""
import numpy as np
import pytest
import torch

import pn2_ref
import util

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
U = {np.float32: 2.0 ** -24, np.float64: 2.0 ** -53}       # unit roundoff


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_pn2_ops")


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_pn2ssg")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def rows(a, transpose):
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if transpose else a


# ------------------------------------------------------------------------------------------------ farthest point sampling

# (B, D, N, M): (a) tail lanes, (b) 2-D, (c) every point / smallest block, then one size per register path (1, 2, 4, 8, 16
# points per lane; float64 leaves the registers above 8 192 points) and (d) the workspace path in both dtypes
FPS_RANDOM = [(3, 3, 1025, 129), (2, 2, 1024, 128), (2, 3, 16, 16), (2, 3, 1, 1), (1, 3, 2049, 24), (1, 2, 5000, 24),
              (1, 3, 8193, 24), (2, 3, 16384, 16), (1, 3, 20000, 64)]


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b, d, n, m", FPS_RANDOM)
def test_fps_equals_the_restatement_on_random_clouds(ops, b, d, n, m, dtype):
    pts = np.random.default_rng(n + d).random((b, n, d)).astype(dtype)
    got = ops.fps(dev(pts), m)
    assert got.dtype == torch.int64 and not got.requires_grad
    assert np.array_equal(host(got), pn2_ref.fps_batch(pts, m))


@pytest.mark.parametrize("dtype", DTYPES)
def test_fps_breaks_ties_like_the_reference_schedule_and_repeats_when_exhausted(ops, dtype):
    for n, m, seed in pn2_ref.LATTICE_CASES:
        pts = pn2_ref.lattice_cloud(n, seed).astype(dtype)
        want = pn2_ref.fps_literal(pts, m)
        got = host(ops.fps(dev(pts[None]), m))[0]
        assert np.array_equal(got, want), (n, np.nonzero(got != want)[0][:5])
        assert np.array_equal(want, pn2_ref.fps_closed(pts, m))
    # the 1 100-point cloud, as the batch of a larger call and through the drop-in's (B, 3, N) layout
    n, m, seed = pn2_ref.LATTICE_CASES[0]
    pts = np.stack([pn2_ref.lattice_cloud(n, seed + i).astype(dtype) for i in range(3)])
    want = pn2_ref.fps_batch(pts, m)
    assert want[0, -1] == want[0, -2]                                  # exhausted: the index is repeated
    import mvkpconv
    fps_mod = mvkpconv.sub("dropin.mvpnet.ops.fps")
    assert np.array_equal(host(fps_mod.farthest_point_sample(dev(pts).transpose(1, 2), m)), want)
    assert np.array_equal(host(fps_mod.farthest_point_sample(dev(pts), m, transpose=False)), want)


def test_fps_reproduces_the_reference_restatement(ops, g15):
    for i in range(4):
        for tag in ("f32", "f64"):
            pts = rows(g15["fps%d_%s_points" % (i, tag)], bool(g15["fps%d_transpose" % i]))
            want = g15["fps%d_%s_index" % (i, tag)]
            assert np.array_equal(host(ops.fps(dev(pts), want.shape[1])), want)


def test_fps_refuses_more_centroids_than_points(ops):
    pts = dev(np.zeros((1, 8, 3), np.float32))
    with pytest.raises(RuntimeError, match="centroids"):
        ops.fps(pts, 9)
    with pytest.raises(RuntimeError, match="centroids"):
        ops.fps(pts, 0)
    with pytest.raises(RuntimeError, match="2-D and 3-D"):
        ops.fps(dev(np.zeros((1, 8, 4), np.float32)), 2)


# ------------------------------------------------------------------------------------------------ ball query

def check_ball_query(ops, q, ky, radius, k):
    want_i, want_d = pn2_ref.ball_query(q, ky, radius, k)
    got_i, got_d = ops.pn2_ball_query(dev(q), dev(ky), radius, k, with_distance=True)
    assert got_i.dtype == torch.int64 and not got_i.requires_grad and not got_d.requires_grad
    assert np.array_equal(host(got_i), want_i)
    assert util.bits_equal(host(got_d), want_d)
    assert np.array_equal(host(ops.pn2_ball_query(dev(q), dev(ky), radius, k)), want_i)
    return want_i


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_ball_query_replays_the_reference_cases_in_both_layouts(ops, dropin, g15, tag):
    bq = dropin("dropin.mvpnet.ops.ball_query")
    for i in range(4):
        r, k, tr = g15["bq%d_radius_k_transpose" % i]
        q, ky = g15["bq%d_%s_query" % (i, tag)], g15["bq%d_%s_key" % (i, tag)]
        want = check_ball_query(ops, rows(q, bool(tr)), rows(ky, bool(tr)), float(r), int(k))
        assert np.array_equal(want, g15["bq%d_%s_index" % (i, tag)])
        # the drop-in's wrapper in the layout the reference's test feeds
        got_i, got_d = bq.ball_query_distance(dev(q), dev(ky), float(r), int(k), transpose=bool(tr))
        assert np.array_equal(host(got_i), want)
        assert np.array_equal(host(got_d).astype(np.float32), g15["bq%d_%s_distance" % (i, tag)])
        assert np.array_equal(host(bq.ball_query(dev(q), dev(ky), float(r), int(k), transpose=bool(tr))), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_ball_query_truncation_empty_rows_and_single_key(ops, dtype):
    rng = np.random.default_rng(5)
    ky = rng.random((2, 333, 3)).astype(dtype)                        # more than one round of 64 keys, a ragged last one
    q = ky[:, rng.permutation(333)[:70]].copy()
    q[0, 3] = 1000.0                                                    # far from every key: a row of -1
    want = check_ball_query(ops, q, ky, 100.0, 7)                     # every key in range, K < N2: the first K keys
    assert np.array_equal(want[1, 0], np.arange(7)) and np.all(want[0, 3] == -1)
    want = check_ball_query(ops, q, ky, 0.25, 16)                     # hits spread over the rounds, some rows padded
    assert (want[..., -1] == want[..., 0]).any() and (want[..., -1] != want[..., 0]).any()
    check_ball_query(ops, q, ky, 0.25, 200)                           # K beyond one round of lanes
    want = check_ball_query(ops, q, ky[:, :1].copy(), 0.6, 4)         # N2 = 1
    assert set(np.unique(want).tolist()) <= {-1, 0}


# ------------------------------------------------------------------------------------------------ 3-NN

def check_knn(ops, q, ky):
    want_i, want_d = pn2_ref.knn3(q, ky)
    got_i, got_d = ops.knn_distance(dev(q), dev(ky), 3)
    assert got_i.dtype == torch.int64 and not got_i.requires_grad and not got_d.requires_grad
    assert np.array_equal(host(got_i), want_i)
    assert util.bits_equal(host(got_d), want_d)
    return want_i, want_d


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_knn_replays_the_reference_cases(ops, dropin, g15, tag):
    knn = dropin("dropin.mvpnet.ops.knn_distance")
    for i in range(4):
        tr = bool(g15["knn%d_transpose" % i])
        q, ky = g15["knn%d_%s_query" % (i, tag)], g15["knn%d_%s_key" % (i, tag)]
        want_i, _ = check_knn(ops, rows(q, tr), rows(ky, tr))
        assert np.array_equal(want_i, g15["knn%d_%s_index" % (i, tag)])
        got_i, got_d = knn.knn_distance(dev(q), dev(ky), 3, transpose=tr)
        assert np.array_equal(host(got_i), want_i)
        np.testing.assert_allclose(host(got_d), g15["knn%d_%s_distance" % (i, tag)], rtol=0, atol=1e-6)   # the reference test's


@pytest.mark.parametrize("dtype", DTYPES)
def test_knn_tie_order_three_keys_and_refusals(ops, dtype):
    rng = np.random.default_rng(9)
    base = rng.integers(0, 4, size=(2, 150, 3)).astype(dtype)         # lattice keys: equal distances everywhere
    ky = np.concatenate([base, base, base[:, :40]], axis=1)           # and every key at least twice, across key tiles
    q = rng.integers(0, 4, size=(2, 300, 3)).astype(dtype)
    want_i, want_d = check_knn(ops, q, ky)
    tied = want_d[..., 0] == want_d[..., 1]
    assert tied.any() and np.all(want_i[..., 0][tied] < want_i[..., 1][tied])
    check_knn(ops, q, ky[:, :3].copy())                               # N2 = 3: every key, sorted
    with pytest.raises(RuntimeError, match="keys"):
        ops.knn_distance(dev(q), dev(ky[:, :2].copy()), 3)
    with pytest.raises(RuntimeError, match="3-NN"):
        ops.knn_distance(dev(q), dev(ky), 4)


# ------------------------------------------------------------------------------------------------ interpolation

def interp_case(b, c, n1, n2, same_index):
    torch.manual_seed(0)                                              # the draws of the reference's test
    feature = torch.randn(b, c, n1).double()
    index = torch.randint(0, n1, [b, n2, 3]).long()
    weight = torch.rand(b, n2, 3).double()
    weight = weight / weight.sum(dim=2, keepdim=True)
    grad_out = torch.randn(b, c, n2).double()
    if same_index:
        index = torch.full_like(index, n1 // 2)
    return feature.numpy(), index.numpy(), weight.numpy(), grad_out.numpy()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b, c, n1, n2, same_index", [(2, 64, 128, 512, False), (3, 65, 129, 513, False),
                                                      (2, 5, 64, 512, True)])
def test_interpolation_forward_and_backward_within_rounding(ops, b, c, n1, n2, same_index, dtype):
    f, idx, w, go = interp_case(b, c, n1, n2, same_index)
    f, w, go = f.astype(dtype), w.astype(dtype), go.astype(dtype)
    wide = np.float64 if dtype == np.float32 else np.longdouble       # the referee carries more bits than the kernel
    u = U[dtype]
    ft = dev(f).requires_grad_(True)
    out = ops.feature_interpolate(ft, dev(idx), dev(w))
    want, scale = pn2_ref.interpolate_fwd(f, idx, w, wide)
    err = np.abs(host(out.detach()).astype(wide) - want)
    bound = 4 * u * scale                                             # three products and three additions
    print("interpolate fwd %s %s: max err / bound %.3f" % (dtype.__name__, (b, c, n1, n2), float((err / np.maximum(bound, 1e-300)).max())))
    assert np.all(err <= bound)
    out.backward(dev(go))
    want, scale, count = pn2_ref.interpolate_bwd(go, idx, w, n1, wide)
    err = np.abs(host(ft.grad).astype(wide) - want)
    bound = (count[:, None, :] + 1) * u * scale                       # T rounded products summed in T roundings, any order
    print("interpolate bwd %s %s: max err / bound %.3f, most contributions %d"
          % (dtype.__name__, (b, c, n1, n2), float((err / np.maximum(bound, 1e-300)).max()), int(count.max())))
    assert np.all(err <= bound)
    assert np.all(host(ft.grad)[np.broadcast_to(count[:, None, :] == 0, err.shape)] == 0)


def test_interpolation_out_of_range_index_is_an_error_not_a_fault(ops):
    f = dev(np.ones((1, 2, 8), np.float32)).requires_grad_(True)
    w = dev(np.full((1, 4, 3), 1 / 3, np.float32))
    ops.pn2_check_indices()                                 # start from a clear status word
    for bad in (8, -1):
        idx = np.zeros((1, 4, 3), np.int64)
        idx[0, 2, 1] = bad
        out = ops.feature_interpolate(f, dev(idx), w)       # the bad index contributes nothing
        assert np.allclose(host(out.detach())[0, :, 2], 2 / 3) and np.allclose(host(out.detach())[0, :, 0], 1.0)
        with pytest.raises(RuntimeError, match="outside"):
            ops.pn2_check_indices()
        ops.pn2_check_indices()                             # reading clears the word
        out.sum().backward()                                # the backward skips it too, and reports it
        assert np.allclose(host(f.grad)[0, :, 0], 11 / 3) and np.all(host(f.grad)[0, :, 1:] == 0)
        f.grad = None
        with pytest.raises(RuntimeError, match="outside"):
            ops.pn2_check_indices()
    ops.set_pn2_index_check(True)                           # eager mode: the forward itself raises
    try:
        with pytest.raises(RuntimeError, match="outside"):
            ops.feature_interpolate(f, dev(idx), w)
        good = ops.feature_interpolate(f, dev(np.zeros((1, 4, 3), np.int64)), w)
        assert np.allclose(host(good.detach()), 1.0)
    finally:
        ops.set_pn2_index_check(False)


# ------------------------------------------------------------------------------------------------ the network

NET_KW = dict(in_channels=4, num_classes=5, sa_channels=((16, 16, 32), (32, 32, 64)), num_centroids=(64, 16),
              radius=(0.2, 0.4), max_neighbors=(8, 8), fp_channels=((32, 32), (32, 16)), fp_neighbors=(3, 3),
              seg_channels=(16,), dropout_prob=0.0)


def test_pn2ssg_against_the_reference_classes(dropin, g16, monkeypatch):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    seen = {"fps": [], "bq": [], "knn": []}

    def recording(kind, fn):
        def wrapped(*args, **kwargs):
            out = fn(*args, **kwargs)
            seen[kind].append(host(out[0] if isinstance(out, tuple) else out))
            return out
        return wrapped

    monkeypatch.setattr(modules, "farthest_point_sample", recording("fps", modules.farthest_point_sample))
    monkeypatch.setattr(modules, "ball_query", recording("bq", modules.ball_query))
    monkeypatch.setattr(modules, "knn_distance", recording("knn", modules.knn_distance))
    net = PN2SSG(**NET_KW).cuda()
    state = {k[3:]: torch.from_numpy(v) for k, v in g16.items() if k.startswith("sd/")}
    net.load_state_dict(state, strict=True)
    batch = {"points": dev(g16["points"]), "feature": dev(g16["feature"])}
    failures = []

    def indices():
        for kind, calls in seen.items():
            assert len(calls) == 2, kind
            for call, got in enumerate(calls):
                assert np.array_equal(got, g16["%s_%d" % (kind, call)]), "%s call %d" % (kind, call)
            calls.clear()

    net.eval()
    with torch.no_grad():
        out = net(batch)["seg_logit"]
    indices()
    util.referee_check("g16 PN2SSG eval logits", host(out), g16["logit_eval_f32"], g16["logit_eval_f64"], failures=failures)
    net.train()
    out = net(batch)["seg_logit"]
    indices()
    util.referee_check("g16 PN2SSG train logits", host(out.detach()), g16["logit_train_f32"], g16["logit_train_f64"],
                       failures=failures)
    out.square().mean().backward()
    names = [n for n, _ in net.named_parameters()]
    assert sorted(names) == sorted(k[len("grad_f64/"):] for k in g16 if k.startswith("grad_f64/"))
    for name, p in net.named_parameters():
        util.referee_check("g16 PN2SSG grad " + name, host(p.grad), g16["grad_f32/" + name], g16["grad_f64/" + name],
                           failures=failures)
    assert not failures, "\n".join(failures)
    dropin("ops").pn2_check_indices()                       # no interpolation met an index outside its key set


class StandIn2D(torch.nn.Module):
    """Stands for the 2D encoder: {'image': (n,3,h,w)} -> {'feature': (n,c,h,w)}."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def test_mvpnet3d_equals_its_wiring_written_out(ops, dropin):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    torch.manual_seed(3)
    b, nv, h, w, c, n_pts, k = 2, 2, 6, 8, 8, 128, 3
    net_3d = PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                    fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    assert isinstance(net.feat_aggreg, m3.FeatureAggregation) and net.net_3d is net_3d
    batch = {"images": torch.randn(b, nv, 3, h, w).cuda(), "image_xyz": torch.rand(b, nv, h, w, 3).cuda(),
             "knn_indices": torch.randint(0, nv * h * w, (b, n_pts, k)).cuda(), "points": torch.rand(b, 3, n_pts).cuda()}
    with torch.no_grad():
        got = net(batch)["seg_logit"]
        f2d = net.net_2d({"image": batch["images"].reshape(b * nv, 3, h, w)})["feature"]
        f2d = f2d.reshape(b, nv, c, h, w).transpose(1, 2).reshape(b, c, nv * h * w)
        xyz = batch["image_xyz"].permute(0, 4, 1, 2, 3).reshape(b, 3, nv * h * w)
        fused = net.feat_aggreg(ops.group_points(xyz, batch["knn_indices"]), batch["points"],
                                ops.group_points(f2d, batch["knn_indices"]))
        want = net_3d({"points": batch["points"], "feature": fused})["seg_logit"]
    assert got.shape == (b, 5, n_pts)
    assert torch.equal(got, want)                           # the same kernels on the same values, no atomics
    assert callable(net.get_loss) and callable(net.get_metric)
