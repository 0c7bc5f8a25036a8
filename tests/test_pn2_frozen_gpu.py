"""GPU: the frozen PointNet++ inference path. Operator level: ops.pn2_sa_mlp_max / ops.pn2_fp_mlp (csrc/pn2_mlp.hip)
against the float64 NumPy restatement of tests/pn2_frozen_ref.py, fed the same index tensor, under the referee rule
err(kernel, f64) <= REFEREE_FACTOR x err(unfused float32 torch ops, f64) + one float32 spacing. Network level:
freeze_inference on the g16 PointNet++ and on the small MVPNet3D of test_chunk_gpu.py against the unfrozen forward and a
float64 forward of the same modules. Points lie on multiples of 2^-6, so farthest point sampling, ball query and 3-NN
pick the same indices in float32 and float64."""
import copy

import numpy as np
import pytest
import torch

import pn2_frozen_ref as ref
from util import REFEREE_FACTOR, bits_equal, check_err, l2_err

pytestmark = pytest.mark.gpu

F32_SPACING = 2.0 ** -23
NET_KW = dict(in_channels=4, num_classes=5, sa_channels=((16, 16, 32), (32, 32, 64)), num_centroids=(64, 16),
              radius=(0.2, 0.4), max_neighbors=(8, 8), fp_channels=((32, 32), (32, 16)), fp_neighbors=(3, 3),
              seg_channels=(16,), dropout_prob=0.0)


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


def chain_params(widths, rng):
    """Packed float32 chain with weights ~ N(0, 1/fan_in) and biases 0.1 N(0, 1)."""
    layers = [(rng.standard_normal((widths[l + 1], widths[l])) / np.sqrt(widths[l]), 0.1 * rng.standard_normal(widths[l + 1]))
              for l in range(len(widths) - 1)]
    return ref.pack(layers).astype(np.float32)


def torch_chain(x, params, widths, relu_last=True):
    """The unfused float32 chain on (B,C,L): one matrix product, bias and ReLU launch per layer."""
    off = 0
    for l in range(len(widths) - 1):
        cin, cout = widths[l], widths[l + 1]
        w = params[off:off + cout * cin].view(cout, cin)
        off += cout * cin
        x = torch.matmul(w, x) + params[off:off + cout].view(1, cout, 1)
        off += cout
        if relu_last or l + 2 < len(widths):
            x = torch.relu(x)
    return x


def referee(label, got, unfused, f64):
    e_ref = l2_err(unfused, f64)
    check_err("%s: fused vs float64 (unfused float32 vs float64: %.3e)" % (label, e_ref), l2_err(got, f64),
              REFEREE_FACTOR * e_ref + F32_SPACING)


# ------------------------------------------------------------------------------------------------ set abstraction

# (B, N, M, K, C, use_xyz, widths after the input, what). Together: K in {1, 5, 16, 32, 33}, M in {1, 7, 64, 130}, B in
# {1, 3}, rows of 3, 1 + 3, 6 + 3, 64 + 3 and 256 + 3 values, chains of one, two and three layers, and every path of the
# host's tile choice: several centroids per 32-row tile, K = 33 in one 64-row tile, K = 33 in two passes of 32 rows (the
# wide chain leaves no room for 64), K = 130 in two passes of 128, and the 64- and 128-row tiles of large grids.
SA_CASES = [
    (1, 50, 1, 1, 0, True, (20,), ""),
    (3, 40, 7, 5, 1, True, (32, 33), ""),
    (1, 100, 64, 16, 6, True, (256, 256, 512), ""),
    (3, 200, 130, 32, 64, True, (32, 33), ""),
    (1, 300, 7, 33, 256, True, (256, 256, 512), ""),
    (1, 90, 7, 33, 1, True, (32, 33), ""),
    (1, 150, 3, 130, 1, True, (20,), ""),
    (1, 5, 7, 32, 6, True, (20,), "repeats"),
    (3, 60, 64, 5, 6, False, (32, 33), ""),
    (1, 80, 130, 16, 6, True, (32, 33), "minus"),
    (1, 80, 7, 32, 64, True, (20,), "negative"),
    (1, 3000, 1200, 32, 6, True, (32, 33), ""),
    (1, 3000, 2100, 32, 6, True, (20,), ""),
]


@pytest.mark.parametrize("b, n, m, k, c, use_xyz, mlp, what", SA_CASES)
def test_set_abstraction_against_the_float64_restatement(ops, b, n, m, k, c, use_xyz, mlp, what):
    rng = np.random.default_rng(1000 + 7 * n + m + k)
    xyz = rng.random((b, 3, n)).astype(np.float32)
    feature = rng.standard_normal((b, c, n)).astype(np.float32) if c else None
    new_xyz = rng.random((b, 3, m)).astype(np.float32)
    index = rng.integers(0, n, size=(b, m, k)).astype(np.int64)
    widths = ((c + 3) if (use_xyz or not c) else c,) + tuple(mlp)
    params = chain_params(widths, rng)
    if what == "repeats":               # a ball query with fewer hits than slots: the first hit fills the rest
        hits = rng.integers(1, n + 1, size=(b, m))
        index = np.where(np.arange(k)[None, None, :] < hits[..., None], index, index[..., :1])
    if what == "minus":                 # rows of -1: a whole centroid, a tail, and a value past the keys
        index[0, 3] = -1
        index[0, 64, 5:] = -1
        index[0, 129, 1] = n + 2
    if what == "negative":              # every pre-activation negative: the max over ReLU outputs is exactly 0
        feature = np.abs(feature)
        layers = ref.unpack(params, widths)
        w = -np.abs(layers[0][0])
        w[:, c:] = 0
        params = ref.pack([(w, -np.abs(layers[0][1]) - 0.01)]).astype(np.float32)
    d = [dev(xyz), None if feature is None else dev(feature), dev(new_xyz), dev(index), dev(params)]
    got = ops.pn2_sa_mlp_max(d[0], d[1], d[2], d[3], d[4], widths)
    assert got.shape == (b, widths[-1], m) and got.dtype == torch.float32
    # unfused: group, subtract, concatenate, the chain, max
    gx = ops.group_points(d[0], d[3]) - d[2].unsqueeze(-1)
    x = gx if feature is None else ops.group_points(d[1], d[3])
    if feature is not None and use_xyz:
        x = torch.cat([x, gx], dim=1)
    unfused = torch_chain(x.reshape(b, widths[0], m * k), d[4], widths).reshape(b, widths[-1], m, k).max(dim=3)[0]
    f64 = ref.sa_mlp_max(xyz, feature, new_xyz, index, params, widths)
    label = "pn2_sa_mlp_max B=%d N=%d M=%d K=%d rows=%d mlp=%s %s" % (b, n, m, k, widths[0], mlp, what)
    if what == "negative":
        assert not f64.any() and not host(got).any() and not np.signbit(host(got)).any()
        return
    referee(label, host(got), host(unfused), f64)
    if what == "minus":                 # a centroid without neighbours sees the row [0 | -new_xyz] K times
        lone = ref.chain(np.concatenate([np.zeros(c), -new_xyz[0, :, 3].astype(np.float64)])[None], ref.unpack(params, widths))
        np.testing.assert_allclose(host(got)[0, :, 3], lone[0], rtol=1e-5, atol=1e-6)


def test_set_abstraction_refuses_what_the_kernel_does_not_run(ops):
    z = lambda *s: torch.zeros(*s, device="cuda")
    idx = torch.zeros(1, 4, 2, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="layers"):
        ops.pn2_sa_mlp_max(z(1, 3, 8), None, z(1, 3, 4), idx, z(4 * 4 + 3 * 4 * 5), (3, 4, 4, 4, 4))
    with pytest.raises(RuntimeError, match="K = 0"):
        ops.pn2_sa_mlp_max(z(1, 3, 8), None, z(1, 3, 4), idx[:, :, :0].contiguous(), z(16), (3, 4))
    with pytest.raises(RuntimeError, match="wide"):
        ops.pn2_sa_mlp_max(z(1, 3, 8), None, z(1, 3, 4), idx, z(4 * 513), (3, 513))
    with pytest.raises(RuntimeError, match="LDS"):
        ops.pn2_fp_mlp(None, None, None, z(1, 768, 4), z(512 * 769 + 512 * 513), (768, 512, 512))
    with pytest.raises(RuntimeError, match="widths"):
        ops.pn2_sa_mlp_max(z(1, 3, 8), z(1, 2, 8), z(1, 3, 4), idx, z(4 * 5), (4, 4))


# ------------------------------------------------------------------------------------------------ propagation and head

# (B, N2, N1, C2, C1, widths after the input, what): N1 in {1, 63, 64, 65, 1000}, rows of 512 + 256 and of 5 + 0 values,
# an index outside the keys, and a grid large enough for the 128-row tile.
FP_CASES = [
    (1, 10, 1, 5, 0, (20,), ""),
    (3, 32, 63, 512, 256, (256, 256), ""),
    (1, 32, 64, 5, 0, (32, 33), ""),
    (1, 20, 65, 5, 3, (32, 33), "outside"),
    (3, 128, 1000, 512, 256, (256, 256), ""),
    (1, 100, 66000, 5, 0, (8,), ""),
]


def fp_inputs(rng, b, n2, n1, c2, c1):
    sparse = rng.standard_normal((b, c2, n2)).astype(np.float32)
    dense = rng.standard_normal((b, c1, n1)).astype(np.float32) if c1 else None
    index = rng.integers(0, n2, size=(b, n1, 3)).astype(np.int64)
    weight = rng.random((b, n1, 3)) + 0.05
    weight = (weight / weight.sum(2, keepdims=True)).astype(np.float32)
    return sparse, index, weight, dense


@pytest.mark.parametrize("b, n2, n1, c2, c1, mlp, what", FP_CASES)
def test_propagation_against_the_float64_restatement(ops, b, n2, n1, c2, c1, mlp, what):
    rng = np.random.default_rng(2000 + n1 + c2)
    sparse, index, weight, dense = fp_inputs(rng, b, n2, n1, c2, c1)
    if what == "outside":
        index[0, 7, 1] = -1
        index[0, 64, 2] = n2
    widths = (c2 + c1,) + tuple(mlp)
    params = chain_params(widths, rng)
    d = [dev(sparse), dev(index), dev(weight), None if dense is None else dev(dense), dev(params)]
    ops.pn2_check_indices()
    got = ops.pn2_fp_mlp(d[0], d[1], d[2], d[3], d[4], widths)
    assert got.shape == (b, widths[-1], n1)
    if what == "outside":               # the status word is set as by feature_interpolate, and read back here
        with pytest.raises(RuntimeError, match="outside the key set"):
            ops.pn2_check_indices()
    x = ops.feature_interpolate(d[0], d[1], d[2])
    if dense is not None:
        x = torch.cat([x, d[3]], dim=1)
    unfused = torch_chain(x, d[4], widths)
    if what == "outside":
        with pytest.raises(RuntimeError, match="outside the key set"):
            ops.pn2_check_indices()
    f64 = ref.fp_mlp(sparse, index, weight, dense, params, widths)
    referee("pn2_fp_mlp B=%d N2=%d N1=%d rows=%d+%d mlp=%s %s" % (b, n2, n1, c2, c1, mlp, what), host(got), host(unfused), f64)


def test_head_form_without_an_index_is_linear_in_its_last_layer(ops):
    rng = np.random.default_rng(31)
    b, n1, widths = 3, 65, (128, 128, 20)
    dense = rng.standard_normal((b, widths[0], n1)).astype(np.float32)
    params = chain_params(widths, rng)
    got = ops.pn2_fp_mlp(None, None, None, dev(dense), dev(params), widths, relu_last=False)
    unfused = torch_chain(dev(dense), dev(params), widths, relu_last=False)
    f64 = ref.fp_mlp(None, None, None, dense, params, widths, relu_last=False)
    assert (f64 < 0).any() and abs(ref.unpack(params, widths)[1][1]).min() > 0       # logits of both signs, a real bias
    referee("pn2_fp_mlp head form 128 -> 128 -> 20", host(got), host(unfused), f64)
    relu = ops.pn2_fp_mlp(None, None, None, dev(dense), dev(params), widths)
    assert bits_equal(host(relu), np.maximum(host(got), np.float32(0)))


@pytest.mark.parametrize("n1", [1, 65, 1000])
def test_interpolated_values_are_bit_equal_to_feature_interpolate(ops, n1):
    """Through a one-layer identity chain without ReLU: fma(1, x, 0) and the zero terms of the other columns are exact."""
    rng = np.random.default_rng(41 + n1)
    c2 = 7
    sparse, index, weight, _ = fp_inputs(rng, 2, 24, n1, c2, 0)
    if n1 > 1:
        index[1, 3, 0] = -5
        index[0, n1 - 1, 2] = 24
    params = ref.pack([(np.eye(c2), np.zeros(c2))]).astype(np.float32)
    d = [dev(sparse), dev(index), dev(weight)]
    got = ops.pn2_fp_mlp(d[0], d[1], d[2], None, dev(params), (c2, c2), relu_last=False)
    want = ops.feature_interpolate(d[0], d[1], d[2])
    if n1 > 1:
        with pytest.raises(RuntimeError, match="outside the key set"):
            ops.pn2_check_indices()
    assert bits_equal(host(got), host(want))


# ------------------------------------------------------------------------------------------------ network level

def dyadic(rng, shape):
    return (rng.integers(0, 64, size=shape) / 64.0).astype(np.float32)


def perturb_batchnorm(net, rng):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                for t, v in ((m.weight, 1 + 0.1 * rng.standard_normal(m.weight.shape)), (m.bias, 0.1 * rng.standard_normal(m.bias.shape)),
                             (m.running_mean, 0.1 * rng.standard_normal(m.bias.shape)),
                             (m.running_var, 1 + 0.1 * np.abs(rng.standard_normal(m.bias.shape)))):
                    t.copy_(torch.from_numpy(v).float())


def g16_net(dropin, golden, **kw):
    """The g16 PointNet++ with its fixture weights (BatchNorm away from the initial values) -- or, with other
    constructor arguments, fresh weights with perturbed BatchNorm -- and a batch of dyadic points."""
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    torch.manual_seed(16)
    net = PN2SSG(**dict(NET_KW, **kw)).cuda()
    if kw:
        perturb_batchnorm(net, np.random.default_rng(16))
    else:
        g16 = golden("g16_pn2ssg")
        net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g16.items() if k.startswith("sd/")}, strict=True)
        assert float(net.sa_modules[0].mlp[0].bn.running_mean.abs().max()) > 0.01
    rng = np.random.default_rng(160)
    batch = {"points": dev(dyadic(rng, (2, 3, 256))), "feature": dev(rng.standard_normal((2, 4, 256)).astype(np.float32))}
    return net.eval(), batch


def float64_forward(net, batch):
    """The same modules in float64 on the device (the pn2 ops have _f64 entry points), never on the frozen path."""
    modules = __import__("mvkpconv").sub("dropin.mvpnet.models.pn2.modules")
    net64 = modules.unfreeze_inference(copy.deepcopy(net)).double().eval()
    with torch.no_grad():
        out = net64({k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()})["seg_logit"]
    assert out.dtype == torch.float64
    return host(out)


class Counted(object):
    """Counts the forwards of the PyTorch layers the frozen path replaces and the calls of the fused ops."""
    LAYERS = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)

    def __init__(self, ops):
        self.ops, self.calls = ops, {"layers": 0, "sa": 0, "fp": 0}

    def __enter__(self):
        self.real = [c.forward for c in self.LAYERS], self.ops.pn2_sa_mlp_max, self.ops.pn2_fp_mlp
        calls = self.calls

        def counting(key, fn):
            def wrapped(*a, **k):
                calls[key] += 1
                return fn(*a, **k)
            return wrapped
        for c, fwd in zip(self.LAYERS, self.real[0]):
            c.forward = counting("layers", fwd)
        self.ops.pn2_sa_mlp_max, self.ops.pn2_fp_mlp = counting("sa", self.real[1]), counting("fp", self.real[2])
        return calls

    def __exit__(self, *exc):
        for c, fwd in zip(self.LAYERS, self.real[0]):
            c.forward = fwd
        self.ops.pn2_sa_mlp_max, self.ops.pn2_fp_mlp = self.real[1], self.real[2]


@pytest.mark.parametrize("variant", ["g16", "fallthrough"])
def test_frozen_pn2ssg_within_the_referee_bound(ops, dropin, golden, variant):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    # fallthrough: the second SetAbstraction is one group of every point and the first FeaturePropagation a broadcast;
    # both stay on the unfrozen path inside a frozen network
    kw = {} if variant == "g16" else dict(num_centroids=(64, 0), fp_neighbors=(0, 3))
    net, batch = g16_net(dropin, golden, **kw)
    keys = list(net.state_dict().keys())
    with torch.no_grad(), Counted(ops) as calls:
        unfrozen = host(net(batch)["seg_logit"])
    assert calls["layers"] > 20 and calls["sa"] == calls["fp"] == 0
    modules.freeze_inference(net)
    assert list(net.state_dict().keys()) == keys
    eligible = [m for m in net.modules() if isinstance(m, modules.Freezable) and m._frozen is not None]
    assert len(eligible) == (5 if variant == "g16" else 3)
    with torch.no_grad(), Counted(ops) as calls:
        frozen = host(net(batch)["seg_logit"])
    if variant == "g16":            # the frozen path is the one that ran: no convolution or BatchNorm forward at all
        assert calls == {"layers": 0, "sa": 2, "fp": 3}
    else:                           # 3 conv + 3 BatchNorm of the global SetAbstraction, 2 + 2 of the broadcast propagation
        assert calls == {"layers": 10, "sa": 1, "fp": 2}
    ops.pn2_check_indices()
    f64 = float64_forward(net, batch)
    e_ref = l2_err(unfrozen, f64)
    check_err("frozen PN2SSG %s: frozen logits vs float64 (unfrozen eval forward vs float64: %.3e)" % (variant, e_ref),
              l2_err(frozen, f64), REFEREE_FACTOR * e_ref + F32_SPACING)
    assert e_ref < 1e-3             # float32 and float64 picked the same centroids and neighbours


def test_frozen_path_is_not_taken_with_gradients_and_train_drops_it(ops, dropin, golden):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    ops.set_deterministic(True)
    try:
        net, batch = g16_net(dropin, golden)
        before = net(batch)["seg_logit"].detach().clone()           # gradients enabled
        modules.freeze_inference(net)
        with Counted(ops) as calls:
            out = net(batch)["seg_logit"]                           # frozen, in eval mode, but gradients are enabled
        assert calls["sa"] == calls["fp"] == 0 and calls["layers"] > 20
        assert out.requires_grad and torch.equal(out.detach(), before)
        net.train()
        assert all(m._frozen is None for m in net.modules() if isinstance(m, modules.Freezable))
        net.eval()
        with torch.no_grad(), Counted(ops) as calls:
            again = net(batch)["seg_logit"]
        assert calls["sa"] == calls["fp"] == 0 and torch.equal(again, before)
    finally:
        ops.set_deterministic(False)


def test_frozen_forward_in_a_captured_graph(ops, dropin, golden):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    net, batch = g16_net(dropin, golden)
    modules.freeze_inference(net)
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


def test_predict_whole_scene_with_a_frozen_mvpnet3d(ops, dropin, golden):
    import test_chunk_gpu as tc
    tm = dropin("dropin.mvpnet.test_mvpnet_3d")
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    g17 = golden("g17_mvpnet_chunks")
    torch.manual_seed(3)
    np.random.seed(3)
    c, n_cls, k, nv = 8, 5, 3, 2
    net_3d = pn2ssg.PN2SSG(8, n_cls, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(tc.StandIn2D(c), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction="sum",
                      use_relation=True).cuda().eval()
    perturb_batchnorm(net, np.random.default_rng(17))
    p = g17["points"]
    assert np.array_equal(p * 64, np.round(p * 64))
    pts = dev(p)
    frames = tc.synthetic_frames(p)
    indices, boxes = tc.chunks_on_device(dropin, p, int(g17["thresholds"][0]))
    inputs = [tm.chunk_rgbd_inputs(pts, ind, box, frames, nv, k=k) for ind, box in zip(indices, boxes)]
    batches = [{key: d[key].unsqueeze(0) for key in ("points", "images", "image_xyz", "knn_indices")} for d in inputs]

    with torch.no_grad():
        unfrozen = host(net(batches[2])["seg_logit"])
    keys = list(net.state_dict().keys())
    assert pn2ssg.freeze_inference(net) is net and list(net.state_dict().keys()) == keys    # reached through net_3d
    assert net_3d.sa_modules[0]._frozen[1] == (11, 16, 16) and net_3d.fp_modules[0]._frozen[1] == (16, 16)
    assert net_3d._frozen[1] == (16, 16, 5)
    with torch.no_grad(), Counted(ops) as calls:
        frozen = net(batches[2])["seg_logit"]
    assert calls["sa"] == 1 and calls["fp"] == 2
    # one chunk against the float64 forward of the whole MVPNet3D
    net64 = pn2ssg.unfreeze_inference(copy.deepcopy(net)).double().eval()
    with torch.no_grad():
        f64 = host(net64({key: (v.double() if v.is_floating_point() else v) for key, v in batches[2].items()})["seg_logit"])
    e_ref = l2_err(unfrozen, f64)
    check_err("frozen MVPNet3D chunk: frozen logits vs float64 (unfrozen eval forward vs float64: %.3e)" % e_ref,
              l2_err(host(frozen), f64), REFEREE_FACTOR * e_ref + F32_SPACING)
    assert e_ref < 1e-3

    # the whole scene: the frozen model handed to predict_whole_scene against chunk-by-chunk frozen forwards
    with Counted(ops) as calls:
        pred, mean = tm.predict_whole_scene(net, pts, inputs, min_nb_pts=64)
    assert calls["sa"] == len(inputs) and calls["fp"] == 2 * len(inputs) and net_3d._frozen is not None
    sums = torch.zeros((len(p), n_cls), device="cuda")
    visits = torch.zeros((len(p),), dtype=torch.int32, device="cuda")
    with torch.no_grad():
        for d, batch in zip(inputs, batches):
            logit = net(batch)["seg_logit"][0]
            sums.index_add_(0, d["chunk_ind"], logit.t().contiguous())
            visits.index_add_(0, d["chunk_ind"], torch.ones_like(d["chunk_ind"], dtype=torch.int32))
    sums, visits = host(sums), host(visits)
    want_mean = sums / np.maximum(visits, 1)[:, None].astype(np.float32)
    want_pred = np.argmax(want_mean, axis=1)
    want_pred[visits == 0] = n_cls
    assert bits_equal(host(mean), want_mean) and np.array_equal(host(pred), want_pred)
    ops.pn2_check_indices()
