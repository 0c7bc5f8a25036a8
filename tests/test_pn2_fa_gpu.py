"""GPU: the fused frozen FeatureAggregation. Operator level: ops.pn2_fa_mlp (pn2_fa_k of csrc/pn2_mlp.hip) against the
float64 NumPy restatement of tests/pn2_fa_ref.py on the same indices, under the referee rule of DESIGN 7j,
err(kernel, f64) <= REFEREE_FACTOR x err(unfused float32 torch ops, f64) + one float32 spacing; bit-equality between
memory layouts, batch sizes, tile sizes and `lengths`. Module level: freeze_inference(net, aggregation=True) on a small
MVPNet3D against the unfrozen forward and the float64 forward, call counts, fall-backs, a captured graph, and
predict_whole_scene_grouped."""
import copy

import numpy as np
import pytest
import torch

import chunk_ref
import pn2_fa_ref as ref
import pn2_frozen_ref as fref
import util
from util import REFEREE_FACTOR, bits_equal

pytestmark = pytest.mark.gpu

H, W = 3, 5                             # a pixel plane that is no multiple of 4


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


@pytest.fixture(scope="module")
def tf():
    import test_pn2_frozen_gpu
    return test_pn2_frozen_gpu


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def fa_inputs(rng, b, nv, c, n, k, h=H, w=W):
    fmap = rng.standard_normal((b * nv, c, h, w)).astype(np.float32)
    image_xyz = rng.random((b, nv, h, w, 3)).astype(np.float32)
    points = rng.random((b, 3, n)).astype(np.float32)
    index = rng.integers(0, nv * h * w, size=(b, n, k)).astype(np.int64)
    return fmap, image_xyz, points, index


def unfused(ops, tf, fmap, image_xyz, points, index, params, widths, reduction, use_relation):
    """MVPNet3D.forward's own float32 steps: transposed copy, two group_points, concatenation, one product, bias and ReLU
    launch per layer, reduction over k."""
    b, nv, h, w, _ = image_xyz.shape
    n, k = index.shape[1:]
    f = fmap.reshape(b, nv, -1, h, w).transpose(1, 2).contiguous().reshape(b, -1, nv * h * w)
    x = ops.group_points(f, index)
    if use_relation:
        xyz = image_xyz.permute(0, 4, 1, 2, 3).reshape(b, 3, nv * h * w).contiguous()
        diff = ops.group_points(xyz, index) - points.unsqueeze(-1)
        x = torch.cat([x, diff, torch.sum(diff ** 2, dim=1, keepdim=True)], dim=1)
    y = tf.torch_chain(x.reshape(b, widths[0], n * k), params, widths).reshape(b, widths[-1], n, k)
    return y.sum(3) if reduction == "sum" else y.max(3)[0]


# (B, nv, C, N, K, widths after the input, reduction, use_relation, what). Together: K in {1, 3, 5, 32, 33, 128} (33 forces
# a 64-row tile, 128 the largest), N in {1, 9, 10, 11, 21, 22, 1000, 2100} (10 / 11 and 21 / 22 straddle the points of a
# 32-row tile at K = 3) plus 11 000 and 22 000, whose B N K rows make the host choose 64- and 128-row tiles at K = 3
# (21 and 42 points per tile), B in {1, 3}, nv in {1, 2, 3}, C in {1, 7, 8, 64} (C + 4 = 11: scalar weight loads, 12: vector
# ones), one to three layers, widths that are no multiple of 16, sum and max, relation off.
FA_CASES = [
    (1, 1, 1, 1, 1, (20,), "sum", True, ""),
    (3, 2, 7, 9, 3, (32, 33), "sum", True, ""),
    (1, 3, 8, 10, 3, (16,), "sum", True, ""),
    (1, 3, 8, 11, 3, (16,), "max", True, ""),
    (3, 2, 64, 21, 5, (64, 64, 64), "sum", True, ""),
    (1, 1, 7, 22, 32, (32, 33), "sum", True, ""),
    (1, 2, 8, 9, 33, (20,), "max", True, ""),
    (1, 3, 1, 21, 128, (24, 40), "sum", True, ""),
    (1, 3, 64, 1000, 3, (64, 64, 64), "sum", True, "outside"),
    (3, 2, 8, 2100, 3, (33,), "sum", False, ""),
    (1, 2, 7, 22, 5, (20,), "max", False, "outside"),
    (1, 3, 8, 11000, 3, (16, 8), "sum", True, ""),
    (1, 2, 8, 22000, 3, (8,), "max", True, ""),
    (1, 2, 7, 10, 5, (20,), "sum", True, "negative"),
]


@pytest.mark.parametrize("b, nv, c, n, k, mlp, reduction, use_relation, what", FA_CASES)
def test_aggregation_against_the_float64_restatement(ops, tf, b, nv, c, n, k, mlp, reduction, use_relation, what):
    rng = np.random.default_rng(3000 + 7 * n + 3 * k + c)
    fmap, image_xyz, points, index = fa_inputs(rng, b, nv, c, n, k)
    p = nv * H * W
    widths = (c + (4 if use_relation else 0),) + tuple(mlp)
    params = tf.chain_params(widths, rng)
    if what == "outside":               # -1 and indices past the pixels: a tail, a whole point, single slots
        index[0, 3] = -1
        index[0, n // 2, 1:] = p
        index[0, n - 1, 0] = p + 7
        index[0, 5, k - 1] = -1
    if what == "negative":              # every pre-activation negative: the sum over ReLU outputs is exactly 0
        fmap = np.abs(fmap)
        layers = fref.unpack(params, widths)
        w0 = -np.abs(layers[0][0])
        w0[:, c:c + 3] = 0              # the differences have both signs; the squared distance does not
        params = fref.pack([(w0, -np.abs(layers[0][1]) - 0.01)]).astype(np.float32)
    d = [dev(fmap), dev(image_xyz), dev(points), dev(index), dev(params)]
    got = ops.pn2_fa_mlp(*d, widths, reduction=reduction, use_relation=use_relation)
    assert got.shape == (b, widths[-1], n) and got.dtype == torch.float32
    # the same map channels-last, read in place: the same loads, so the same bits
    cl = d[0].contiguous(memory_format=torch.channels_last)
    assert c == 1 or not cl.is_contiguous()
    got_cl = ops.pn2_fa_mlp(cl, *d[1:], widths, reduction=reduction, use_relation=use_relation)
    assert bits_equal(host(got_cl), host(got))
    f64 = ref.fa_mlp(fmap, image_xyz, points, index, params, widths, reduction=reduction, use_relation=use_relation)
    label = "pn2_fa_mlp B=%d nv=%d C=%d N=%d K=%d mlp=%s %s%s %s" % (b, nv, c, n, k, mlp, reduction,
                                                                    "" if use_relation else " no relation", what)
    if what == "negative":
        assert not f64.any() and not host(got).any() and not np.signbit(host(got)).any()
        return
    tf.referee(label, host(got), host(unfused(ops, tf, *d, widths, reduction, use_relation)), f64)
    if what == "outside":               # a point without a pixel sees the row [0 | -point | |point|^2] K times
        pt = points[0, :, 3].astype(np.float64)
        row = np.concatenate([np.zeros(c), -pt, [pt @ pt]])[:widths[0]]
        lone = fref.chain(row[None], fref.unpack(params, widths))[0] * (k if reduction == "sum" else 1)
        np.testing.assert_allclose(host(got)[0, :, 3], lone, rtol=1e-5, atol=1e-6)


def test_a_point_does_not_depend_on_the_batch_or_the_tile(ops, tf):
    """The same cloud alone (3 000 rows: 32-row tiles, 10 points each) and as one of 12 and of 24 (36 000 and 72 000 rows:
    64- and 128-row tiles, 21 and 42 points each), sum and max."""
    rng = np.random.default_rng(61)
    nv, c, n, k, widths = 2, 8, 1000, 3, (12, 16, 8)
    fmap, image_xyz, points, index = fa_inputs(rng, 24, nv, c, n, k)
    params = dev(tf.chain_params(widths, rng))
    d = [dev(fmap), dev(image_xyz), dev(points), dev(index)]
    for reduction in ("sum", "max"):
        big = host(ops.pn2_fa_mlp(*d, params, widths, reduction=reduction))
        for i, nb in ((5, 12), (5, 1), (23, 1)):
            part = [d[0][i * nv:(i + nb) * nv].contiguous()] + [t[i:i + nb].contiguous() for t in d[1:]]
            assert bits_equal(host(ops.pn2_fa_mlp(*part, params, widths, reduction=reduction)), big[i:i + nb]), (reduction, i, nb)


def test_aggregation_refuses_what_the_kernel_does_not_run(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")

    def call(k=3, widths=(8, 4), n_params=None):
        need = sum(widths[i + 1] * (widths[i] + 1) for i in range(len(widths) - 1))
        return ops.pn2_fa_mlp(z(2, 4, H, W), z(1, 2, H, W, 3), z(1, 3, 6), torch.zeros(1, 6, k, dtype=torch.int64, device="cuda"),
                              z(need if n_params is None else n_params), widths)
    assert call().shape == (1, 4, 6)
    assert call(k=128).shape == (1, 4, 6)
    with pytest.raises(RuntimeError, match="K = 129"):
        call(k=129)
    with pytest.raises(RuntimeError, match="K = 0"):
        call(k=0)
    with pytest.raises(RuntimeError, match="layers"):
        call(widths=(8, 4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="wide"):
        call(widths=(8, 513))
    with pytest.raises(RuntimeError, match="packed chain"):
        call(n_params=35)
    with pytest.raises(RuntimeError, match="HBM"):              # lengths on the host
        ops.pn2_fa_mlp(z(2, 4, H, W), z(1, 2, H, W, 3), z(1, 3, 6), torch.zeros(1, 6, 3, dtype=torch.int64, device="cuda"),
                       z(36), (8, 4), lengths=torch.ones(1, dtype=torch.int64))


# (B, N, lengths): 32-row tiles hold 10 points at K = 3, 64-row tiles 21, 128-row tiles 42; every batch mixes 1, G, G + 1
# and N for its own tile and has lengths that leave whole tiles behind n_b
LENGTH_CASES = [
    (8, 50, [1, 10, 11, 21, 22, 42, 43, 50]),
    (4, 3000, [21, 22, 1, 3000]),
    (8, 3000, [42, 43, 1, 3000, 10, 11, 2999, 84]),
]


@pytest.mark.parametrize("reduction", ["sum", "max"])
@pytest.mark.parametrize("b, n, lengths", LENGTH_CASES)
def test_lengths_cut_each_cloud_and_zero_the_rest(ops, tf, b, n, lengths, reduction):
    rng = np.random.default_rng(71 + n)
    nv, c, k, widths = 2, 8, 3, (12, 16, 9)
    fmap, image_xyz, points, index = fa_inputs(rng, b, nv, c, n, k)
    params = dev(tf.chain_params(widths, rng))
    full = host(ops.pn2_fa_mlp(dev(fmap), dev(image_xyz), dev(points), dev(index), params, widths, reduction=reduction))
    for i, nb in enumerate(lengths):    # behind n_b: NaN points and indices far outside any buffer
        points[i, :, nb:] = np.nan
        index[i, nb:] = 1 << 40
    d = [dev(fmap), dev(image_xyz), dev(points), dev(index)]
    got = host(ops.pn2_fa_mlp(*d, params, widths, reduction=reduction, lengths=dev(np.asarray(lengths, np.int64))))
    for i, nb in enumerate(lengths):
        alone = ops.pn2_fa_mlp(d[0][i * nv:(i + 1) * nv], d[1][i:i + 1], d[2][i:i + 1, :, :nb].contiguous(),
                               d[3][i:i + 1, :nb].contiguous(), params, widths, reduction=reduction)
        assert bits_equal(got[i, :, :nb], host(alone)[0]), (i, nb)
        assert bits_equal(got[i, :, :nb], full[i, :, :nb]), (i, nb)
        assert not got[i, :, nb:].any() and not np.signbit(got[i, :, nb:]).any(), (i, nb)
    # lengths = N is the call without lengths; 0 and negative counts clamp to 1, counts above N to N
    clean = [dev(fmap), dev(image_xyz), dev(np.nan_to_num(points)), dev(np.where(index > (1 << 39), 0, index))]
    plain = host(ops.pn2_fa_mlp(*clean, params, widths, reduction=reduction))
    same = host(ops.pn2_fa_mlp(*clean, params, widths, reduction=reduction, lengths=dev(np.full(b, n, np.int64))))
    assert bits_equal(same, plain)
    clamp = np.asarray([0, -5, n + 7] + [n] * (b - 3), np.int64)
    clamped = host(ops.pn2_fa_mlp(*clean, params, widths, reduction=reduction, lengths=dev(clamp)))
    assert bits_equal(clamped[2:], plain[2:]) and bits_equal(clamped[:2, :, :1], plain[:2, :, :1]) and not clamped[:2, :, 1:].any()


# ------------------------------------------------------------------------------------------------ module level

class Calls(object):
    """Counts, beside tf.Counted's layers / sa / fp, the calls of ops.pn2_fa_mlp and ops.group_points."""

    def __init__(self, ops, tf):
        self.ops, self.inner, self.n = ops, tf.Counted(ops), {"fa": 0, "group": 0}

    def __enter__(self):
        calls = self.inner.__enter__()
        self.real = self.ops.pn2_fa_mlp, self.ops.group_points
        n = self.n

        def counting(key, fn):
            def wrapped(*a, **kw):
                n[key] += 1
                return fn(*a, **kw)
            return wrapped
        self.ops.pn2_fa_mlp, self.ops.group_points = counting("fa", self.real[0]), counting("group", self.real[1])
        self.n.update(calls)
        self.calls = calls
        return self

    def __exit__(self, *exc):
        self.ops.pn2_fa_mlp, self.ops.group_points = self.real
        self.inner.__exit__(*exc)
        self.n.update(self.calls)


def small_mvpnet(dropin, tf, **kw):
    """The small MVPNet3D of test_pn2_frozen_gpu.py with a stand-in encoder, perturbed BatchNorm, and a batch of 3 clouds."""
    import test_chunk_gpu as tc
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    torch.manual_seed(3)
    b, nv, h, w, c, n_pts, k = 3, 2, 6, 8, 8, 128, 3
    net_3d = pn2ssg.PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(tc.StandIn2D(c), None, net_3d, **dict(dict(in_channels=c, mlp_channels=(8, 8), reduction="sum",
                                                                 use_relation=True), **kw)).cuda().eval()
    tf.perturb_batchnorm(net, np.random.default_rng(18))
    rng = np.random.default_rng(19)
    batch = {"images": torch.randn(b, nv, 3, h, w).cuda(), "image_xyz": torch.rand(b, nv, h, w, 3).cuda(),
             "knn_indices": torch.randint(0, nv * h * w, (b, n_pts, k)).cuda(), "points": dev(tf.dyadic(rng, (b, 3, n_pts)))}
    return net, batch, pn2ssg


def float64_logits(net, batch, pn2ssg):
    net64 = pn2ssg.unfreeze_inference(copy.deepcopy(net)).double().eval()
    with torch.no_grad():
        out = net64({key: (v.double() if v.is_floating_point() else v) for key, v in batch.items()})["seg_logit"]
    assert out.dtype == torch.float64
    return host(out)


@pytest.mark.parametrize("reduction", ["sum", "max"])
def test_frozen_aggregation_within_the_referee_bound(ops, dropin, tf, reduction):
    net, batch, pn2ssg = small_mvpnet(dropin, tf, reduction=reduction)
    keys = list(net.state_dict().keys())
    with torch.no_grad(), Calls(ops, tf) as c0:
        unfrozen = host(net(batch)["seg_logit"])
    assert c0.n["fa"] == 0 and c0.n["group"] >= 2 and c0.n["layers"] > 5
    pn2ssg.freeze_inference(net)                                 # the one-argument call: the 3D network only
    assert net.feat_aggreg._frozen is None
    with torch.no_grad(), Calls(ops, tf) as c1:
        net(batch)
    assert c1.n["fa"] == 0 and c1.n["group"] == 2 and c1.n["layers"] == 1 + 4      # encoder, 2 x (Conv2d + BatchNorm2d)
    pn2ssg.freeze_inference(net, aggregation=True)
    assert net.feat_aggreg._frozen[1:] == ((12, 8, 8), reduction, True) and list(net.state_dict().keys()) == keys
    with torch.no_grad(), Calls(ops, tf) as c2:
        frozen = host(net(batch)["seg_logit"])
    # no group_points, no Conv2d / BatchNorm forward but the stand-in encoder's own convolution, one fused launch
    assert c2.n == {"fa": 1, "group": 0, "layers": 1, "sa": 1, "fp": 2}
    ops.pn2_check_indices()
    f64 = float64_logits(net, batch, pn2ssg)
    e_ref = util.l2_err(unfrozen, f64)
    util.check_err("MVPNet3D, aggregation frozen (%s): frozen logits vs float64 (unfrozen eval forward vs float64: %.3e)"
                   % (reduction, e_ref), util.l2_err(frozen, f64), REFEREE_FACTOR * e_ref + tf.F32_SPACING)
    assert e_ref < 1e-3
    # with lengths: the valid columns of the 3D network's input are those of the call without, the rest zeros
    seen = []
    hook = net.net_3d.register_forward_pre_hook(lambda mod, args: seen.append(args[0]["feature"].clone()))
    try:
        with torch.no_grad():
            net(batch)
            net(dict(batch, lengths=dev(np.asarray([128, 91, 32], np.int64))))
    finally:
        hook.remove()
    for i, nb in enumerate((128, 91, 32)):
        assert torch.equal(seen[1][i, :, :nb], seen[0][i, :, :nb]) and not seen[1][i, :, nb:].any()


def test_fused_path_is_left_with_gradients_training_float64_or_no_mlp(ops, dropin, tf):
    net, batch, pn2ssg = small_mvpnet(dropin, tf)
    ops.set_deterministic(True)
    try:
        before = net(batch)["seg_logit"].detach().clone()       # gradients enabled, nothing frozen
        pn2ssg.freeze_inference(net, aggregation=True)
        with Calls(ops, tf) as c:
            out = net(batch)["seg_logit"]                       # frozen, eval mode, but gradients are enabled
        assert c.n["fa"] == c.n["sa"] == 0 and c.n["group"] >= 2 and out.requires_grad and torch.equal(out.detach(), before)
        # a float64 copy keeps the float32 snapshot and does not use it
        net64 = copy.deepcopy(net).double()
        assert net64.feat_aggreg._frozen is not None
        batch64 = {key: (v.double() if v.is_floating_point() else v) for key, v in batch.items()}
        with torch.no_grad(), Calls(ops, tf) as c:
            out64 = net64(batch64)["seg_logit"]
        assert c.n["fa"] == 0 and out64.dtype == torch.float64 and bits_equal(host(out64), float64_logits(net, batch, pn2ssg))
        net.train()
        assert net.feat_aggreg._frozen is None
        net.eval()
        with torch.no_grad(), Calls(ops, tf) as c:
            again = net(batch)["seg_logit"]
        assert c.n["fa"] == 0 and torch.equal(again, before)
    finally:
        ops.set_deterministic(False)
    # an aggregation without an MLP has nothing to freeze: the forward is the one before
    bare, batch, _ = small_mvpnet(dropin, tf, mlp_channels=())
    with torch.no_grad():
        want = bare(batch)["seg_logit"].clone()
        pn2ssg.freeze_inference(bare, aggregation=True)
        assert bare.feat_aggreg._frozen is None and bare.net_3d._frozen is not None
        with Calls(ops, tf) as c:
            got = bare(batch)["seg_logit"]
        pn2ssg.unfreeze_inference(bare)
        assert c.n["fa"] == 0 and c.n["group"] == 2
        frozen_3d_only = copy.deepcopy(bare)
        pn2ssg.freeze_inference(frozen_3d_only)
        assert torch.equal(got, frozen_3d_only(batch)["seg_logit"]) and util.l2_err(host(got), host(want)) < 1e-5


def test_frozen_aggregation_in_a_captured_graph(ops, dropin, tf):
    net, batch, pn2ssg = small_mvpnet(dropin, tf)
    pn2ssg.freeze_inference(net, aggregation=True)
    batch = dict(batch, lengths=dev(np.asarray([128, 91, 32], np.int64)))
    with torch.no_grad():
        eager = net(batch)["seg_logit"].clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            net(batch)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = net(batch)["seg_logit"]
        for _ in range(2):
            out.zero_()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)


def test_whole_scene_with_the_aggregation_frozen(ops, dropin, tf, golden):
    import test_chunk_gpu as tc
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
    assert sizes[0] < min_nb_pts <= sizes[1]

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

    def scene(g):
        np.random.seed(99)
        pred, mean = wg.predict_whole_scene_grouped(net, pts, inputs, min_nb_pts=min_nb_pts, chunks_per_forward=g)
        return host(pred), host(mean)

    pred0, mean0 = scene(1)                                             # the unfrozen loop
    pn2ssg.freeze_inference(net, aggregation=True)
    failures = []
    for g in (1, 3):
        with Calls(ops, tf) as calls:
            pred, mean = scene(g)
        assert len(inputs) >= calls.n["fa"] >= -(-len(inputs) // g) and calls.n["group"] == 0
        assert g > 1 or calls.n["fa"] == len(inputs)
        util.referee_check("whole scene, aggregation frozen, mean logits at G = %d (reference: unfrozen loop)" % g, mean, mean0,
                           mean64, floor=tf.F32_SPACING, failures=failures)
        # predictions: every visited point is compared, none is left out for a small margin
        diff = np.abs(mean.astype(np.float64) - mean0).max(axis=1)
        top = np.sort(mean0.astype(np.float64), axis=1)
        decided = visited & (top[:, -1] - top[:, -2] > diff)
        msg = "G = %d: largest logit difference %.3e, %d visited points left out" % (g, diff[visited].max(),
                                                                                    int((visited & ~decided).sum()))
        print(msg)
        assert np.array_equal(decided, visited), msg
        assert np.array_equal(pred, pred0), msg
    assert not failures, "\n".join(failures)
    ops.pn2_check_indices()
