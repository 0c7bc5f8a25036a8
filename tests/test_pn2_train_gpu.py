"""GPU: the fused PointNet++ training path. Operator level: ops.pn2_sa_rows / ops.pn2_rows_max (csrc/pn2_rows.hip)
against the NumPy restatement of tests/pn2_train_ref.py -- forwards and the ordered backward bit for bit, the atomic
backward within (T + 1) u sum|g|. Module and network level: fuse_training against the unfused modules and a float64 run
of the same modules under util.referee_check, the g16 PointNet++ against its fixture, bit-reproducibility in
deterministic mode and a captured forward + backward. Points lie on multiples of 2^-6, so farthest point sampling, ball
query and 3-NN pick the same indices in float32 and float64."""
import copy

import numpy as np
import pytest
import torch

import pn2_train_ref as ref
import util
from pn2_ordered_ref import ball_like_index
from util import bits_equal

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
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


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_pn2ssg")


@pytest.fixture
def deterministic(ops):
    ops.set_deterministic(True)
    yield
    ops.set_deterministic(False)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def dyadic(rng, shape):
    return (rng.integers(0, 64, size=shape) / 64.0).astype(np.float32)


# ------------------------------------------------------------------------------------------------ group rows

# (B, N, M, K, C, use_xyz, index). Together: B in {1, 2, 3}, N in {1, 9, 70}, M in {1, 3, 7, 65}, K in {1, 2, 5, 32, 33},
# rows of 3, 4 (+ 3), 8 (+ 3) and 64 (+ 3) values with and without the coordinates; R from 1 to 6 435 (26 workgroups),
# every channel-group count of the forward's grid (1, 4, 8). index: "ball" = a real ball query; "made" = ball-like with
# rows of -1 and pad repeats; "one" = one key owns every position. N = 1 with 8 channels: the feature's channel stride is
# 1, the one shape at which a kernel choice by strides would leave the plane kernels for the channels-last tile.
ROWS_CASES = [(1, 9, 1, 1, None, True, "ball"), (3, 70, 7, 5, 4, True, "ball"), (1, 70, 65, 32, 64, True, "ball"),
              (3, 9, 65, 33, 4, False, "made"), (1, 70, 7, 33, 64, False, "made"), (3, 70, 1, 32, None, True, "made"),
              (3, 9, 7, 5, 64, True, "one"), (1, 9, 65, 1, 4, True, "made"), (3, 70, 65, 33, 64, True, "ball"),
              (2, 1, 3, 2, 8, True, "made")]


def rows_case(ops, b, n, m, k, c, kind, seed):
    rng = np.random.default_rng(seed)
    xyz, new_xyz = dyadic(rng, (b, 3, n)), dyadic(rng, (b, 3, m))
    feature = None if c is None else rng.standard_normal((b, c, n)).astype(np.float32)
    if kind == "ball":
        index = host(ops.pn2_ball_query(dev(new_xyz.transpose(0, 2, 1)), dev(xyz.transpose(0, 2, 1)), 0.45, k))
    elif kind == "made":
        index = ball_like_index(b, m, k, n, seed=seed + 1)
        index[0, 0, 0] = n                                       # one index past the end as well
    else:
        index = np.full((b, m, k), 3, np.int64)
    return xyz, feature, new_xyz, index


@pytest.mark.parametrize("b, n, m, k, c, use_xyz, kind", ROWS_CASES)
def test_rows_forward_and_both_backwards(ops, b, n, m, k, c, use_xyz, kind):
    xyz, feature, new_xyz, index = rows_case(ops, b, n, m, k, c, kind, seed=b * 1000 + n * 10 + m + k)
    want = ref.sa_rows(xyz, feature, new_xyz, index, use_xyz)
    cin, r = want.shape
    assert cin == (c or 0) + (3 if use_xyz or c is None else 0) and r == b * m * k
    rng = np.random.default_rng(99)
    dx = rng.standard_normal((cin, r)).astype(np.float32)
    d_xyz, d_new, d_idx = dev(xyz), dev(new_xyz), dev(index)
    results = {}
    for mode in ("atomic", "ordered", "ordered again"):
        ops.set_deterministic(mode != "atomic")
        try:
            ft = None if feature is None else dev(feature).requires_grad_(True)
            x = ops.pn2_sa_rows(d_xyz, ft, d_new, d_idx, use_xyz=use_xyz)
            assert x.shape == (cin, r) and x.is_contiguous()
            assert bits_equal(host(x), want)                     # a gather and one rounded subtraction
            if ft is None:
                assert not x.requires_grad
                continue
            x.backward(dev(dx))
            results[mode] = host(ft.grad)
        finally:
            ops.set_deterministic(False)
    if feature is None:
        return
    wide, scale, count = ref.sa_rows_bwd_wide(dx, index, c, n)
    err = np.abs(results["atomic"].astype(np.float64) - wide)
    bound = (count[:, None, :] + 1) * U32 * scale                # T rounded additions in any order
    print("pn2_sa_rows atomic bwd %s: max err / bound %.3f, most contributions %d"
          % ((b, n, m, k, c, kind), float((err / np.maximum(bound, 1e-300)).max()), int(count.max())))
    assert np.all(err <= bound)
    empty = np.broadcast_to(count[:, None, :] == 0, err.shape)
    oracle = ref.sa_rows_bwd(dx, index, c, n)
    for mode in ("ordered", "ordered again"):
        assert bits_equal(results[mode], oracle), mode          # acc = fl(acc + g) over ascending positions
        assert not np.signbit(results[mode][empty]).any() and np.all(results[mode][empty] == 0)
    assert np.all(results["atomic"][empty] == 0)


def test_rows_ordered_backward_walks_a_row_longer_than_512(ops, deterministic):
    b, n, m, k, c = 1, 9, 48, 32, 5                              # one key with M*K = 1 536 entries
    rng = np.random.default_rng(3)
    xyz, new_xyz = dyadic(rng, (b, 3, n)), dyadic(rng, (b, 3, m))
    feature = rng.standard_normal((b, c, n)).astype(np.float32)
    index = np.full((b, m, k), 6, np.int64)
    dx = rng.standard_normal((c + 3, b * m * k)).astype(np.float32)
    ft = dev(feature).requires_grad_(True)
    ops.pn2_sa_rows(dev(xyz), ft, dev(new_xyz), dev(index)).backward(dev(dx))
    got, want = host(ft.grad), ref.sa_rows_bwd(dx, index, c, n)
    assert bits_equal(got, want)
    assert np.all(got[:, :, 6] != 0) and not got[:, :, :6].any() and not np.signbit(got[:, :, :6]).any()
    # the order matters on this row: the sum of the same values in descending order is another float
    assert not np.array_equal(want[0, :, 6], ref.sa_rows_bwd(dx[:, ::-1].copy(), index, c, n)[0, :, 6])


def test_rows_and_group_points_share_one_csr(ops, deterministic, monkeypatch):
    rng = np.random.default_rng(8)
    b, n, m, k, c = 2, 40, 9, 5, 4
    index = dev(ball_like_index(b, m, k, n, seed=9))
    built = []
    real = ops.index_csr
    monkeypatch.setattr(ops, "index_csr", lambda *a, **kw: built.append(1) or real(*a, **kw))
    f1 = dev(rng.standard_normal((b, c, n)).astype(np.float32)).requires_grad_(True)
    f2 = dev(rng.standard_normal((b, c, n)).astype(np.float32)).requires_grad_(True)
    xyz, new_xyz = dev(dyadic(rng, (b, 3, n))), dev(dyadic(rng, (b, 3, m)))
    assert ops.index_csr_for(index, n) is None
    ops.pn2_sa_rows(xyz, f1, new_xyz, index).sum().backward()
    csr = ops.index_csr_for(index, n)
    assert csr is not None and len(built) == 1
    ops.group_points(f2, index).sum().backward()
    assert len(built) == 1 and ops.index_csr_for(index, n)[0] is csr[0] and ops.index_csr_for(index, n)[1] is csr[1]
    ops.pn2_sa_rows(xyz, f1, new_xyz, index).sum().backward()
    assert len(built) == 1
    # the same sums from both ops (two backwards of the rows, one of group_points)
    assert np.array_equal(host(f1.grad), 2 * host(f2.grad)) and host(f2.grad).max() >= 2      # counts: exact in float32


def test_rows_refuse_coordinates_that_require_a_gradient(ops):
    xyz = torch.zeros(1, 3, 9, device="cuda", requires_grad=True)
    new_xyz, index = torch.zeros(1, 3, 2, device="cuda"), torch.zeros(1, 2, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="no gradient for coordinates"):
        ops.pn2_sa_rows(xyz, None, new_xyz, index)
    with pytest.raises(RuntimeError, match="no gradient for coordinates"):
        ops.pn2_sa_rows(xyz.detach(), None, new_xyz.requires_grad_(True), index)
    with torch.no_grad():
        assert ops.pn2_sa_rows(xyz, None, new_xyz, index).shape == (3, 6)


# ------------------------------------------------------------------------------------------------ max over the neighbours

# (B, M, K, Cout): Cout in {5, 64, 130} (a part tile, one tile, two tiles and a part), K in {1, 5, 32, 33}, M in {1, 7, 65}
# (a part tile, two tiles and a part), B in {1, 3}
MAX_CASES = [(1, 1, 1, 5), (3, 7, 5, 64), (1, 65, 32, 130), (3, 65, 33, 5), (1, 7, 33, 130), (3, 1, 32, 64), (3, 65, 5, 130)]


@pytest.mark.parametrize("b, m, k, cout", MAX_CASES)
def test_rows_max_forward_and_backward_are_exact(ops, b, m, k, cout):
    rng = np.random.default_rng(b * 100 + m + k + cout)
    y = (np.round(rng.standard_normal((b, m, k, cout)) * 2) / 2).astype(np.float32)      # few values: ties in most groups
    y[:, :, k // 2:] = y[:, :, :1]                                                       # pad repeats of the first row
    y[0, 0] = 0                                                                          # a group of zeros
    if m > 2:
        y[-1, 2] = -0.0
        y[-1, 2, k - 1] = 0.0                                                            # -0 first, +0 later: not greater
    y = y.reshape(b * m * k, cout)
    want, want_arg = ref.rows_max(y, b, m, k)
    yt = dev(y).requires_grad_(True)
    out, arg = ops.pn2_rows_max(yt, b, m, k, return_arg=True)
    assert out.shape == (b, cout, m) and arg.dtype == torch.int32 and not arg.requires_grad
    assert bits_equal(host(out), want) and np.array_equal(host(arg), want_arg)
    t = y.reshape(b, m, k, cout)
    tied = (t == t.max(axis=2, keepdims=True)).sum(axis=2) > 1
    assert k == 1 or (tied.any() and (want_arg == 0).any() and (want_arg > 0).any())     # equal maxima: the lowest k
    g = rng.standard_normal((b, cout, m)).astype(np.float32)
    out.backward(dev(g))
    assert bits_equal(host(yt.grad), ref.rows_max_bwd(g, want_arg, k))                   # g at arg, +0 elsewhere
    assert torch.equal(ops.pn2_rows_max(yt.detach(), b, m, k), out.detach())


def test_rows_max_propagates_nan_like_torch_max(ops):
    rng = np.random.default_rng(12)
    b, m, k, cout = 2, 3, 6, 70
    y = rng.standard_normal((b * m * k, cout)).astype(np.float32)
    y[7, 3] = y[9, 3] = np.nan                                   # group (0, 1): rows 6..11, first NaN at k = 1
    y[35, 69] = np.nan                                           # the last row of the last group
    out, arg = ops.pn2_rows_max(dev(y), b, m, k, return_arg=True)
    want = torch.max(dev(y).view(b, m, k, cout), dim=2)[0].permute(0, 2, 1)
    assert bits_equal(host(out), host(want.contiguous()))
    assert np.isnan(host(out)).sum() == 2 and host(arg)[0, 3, 1] == 1 and host(arg)[1, 69, 2] == 5
    assert np.array_equal(host(arg), ref.rows_max(y, b, m, k)[1])


@pytest.mark.parametrize("trans_a", [False, True])
def test_product_of_more_rows_than_one_grid_takes(ops, trans_a):
    """The rows of the default network's first level at 32 chunks (32 x 2048 x 32 = 2^21, 2^16 row tiles of 32): the
    product runs as row chunks. Small integers: every product and sum is exact in float32, so the float64 product is
    the expected value bit for bit; the last rows sit in a part tile of the last chunk."""
    torch.manual_seed(5)
    rows, kd, n = (1 << 21) + 37, 4, 64
    a = torch.randint(-3, 4, (rows, kd), device="cuda").float()
    w = torch.randint(-3, 4, (n, kd), device="cuda").float()
    want = (a.double() @ w.double().t()).float()
    got = ops.gemm(a.t().contiguous() if trans_a else a, w, transA=trans_a, transB=True)
    assert got.shape == (rows, n) and torch.equal(got, want)
    assert float(want[-1].abs().max()) > 0 and float(want[15 * 65536].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ modules

def perturb_batchnorm(net, rng):
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                for t, v in ((mod.weight, 1 + 0.1 * rng.standard_normal(mod.weight.shape)),
                             (mod.bias, 0.1 * rng.standard_normal(mod.bias.shape)),
                             (mod.running_mean, 0.1 * rng.standard_normal(mod.bias.shape)),
                             (mod.running_var, 1 + 0.1 * np.abs(rng.standard_normal(mod.bias.shape)))):
                    t.copy_(torch.from_numpy(v).float())


def run_module(module, inputs, grad_inputs, go, dtype):
    """One training forward + backward of a copy of `module` in `dtype`: output, input gradients, parameter gradients,
    running statistics and batch counters, all on the host."""
    mod = copy.deepcopy(module).to(dtype).train()
    args = [None if a is None else (a.to(dtype) if a.is_floating_point() else a).clone() for a in inputs]
    for i in grad_inputs:
        args[i].requires_grad_(True)
    out = mod(*args)
    out = out[1] if isinstance(out, tuple) else out
    out.backward(go.to(dtype))
    res = {"output": host(out)}
    for i in grad_inputs:
        res["grad input %d" % i] = host(args[i].grad)
    for name, p in mod.named_parameters():
        res["grad " + name] = host(p.grad)
    counters = {}
    for name, buf in mod.named_buffers():
        if name.endswith("num_batches_tracked"):
            counters[name] = int(buf)
        else:
            res[name] = host(buf)
    return res, counters


def referee_module(label, modules, module, inputs, grad_inputs, go, calls_expected):
    fused_mod = modules.fuse_training(copy.deepcopy(module))
    f64, n64 = run_module(module, inputs, grad_inputs, go, torch.float64)
    unfused, n32 = run_module(module, inputs, grad_inputs, go, torch.float32)
    fused, nf = run_module(fused_mod, inputs, grad_inputs, go, torch.float32)
    assert calls_expected()
    assert sorted(fused) == sorted(unfused) == sorted(f64) and nf == n32 == n64 and all(v == 1 for v in nf.values())
    assert any(k.endswith("running_var") for k in fused) and any(k.startswith("grad mlp.0.conv") for k in fused)
    failures = []
    for key in sorted(fused):
        assert fused[key].shape == f64[key].shape and fused[key].dtype == np.float32
        util.referee_check("%s %s" % (label, key), fused[key], unfused[key], f64[key], failures=failures)
    assert not failures, "\n".join(failures)


class CountedOps(object):
    """Counts the calls of the ops of the fused training path and the forwards of the PyTorch layers it replaces."""
    LAYERS = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)
    OPS = ("pn2_sa_rows", "pn2_rows_max", "group_points", "linear", "bn_lrelu")

    def __init__(self, ops):
        self.ops, self.calls = ops, dict({"layers": 0}, **{k: 0 for k in self.OPS})

    def __enter__(self):
        self.real = [c.forward for c in self.LAYERS], [getattr(self.ops, k) for k in self.OPS]
        calls = self.calls

        def counting(key, fn):
            def wrapped(*a, **k):
                calls[key] += 1
                return fn(*a, **k)
            return wrapped
        for c, fwd in zip(self.LAYERS, self.real[0]):
            c.forward = counting("layers", fwd)
        for k, fn in zip(self.OPS, self.real[1]):
            setattr(self.ops, k, counting(k, fn))
        return calls

    def __exit__(self, *exc):
        for c, fwd in zip(self.LAYERS, self.real[0]):
            c.forward = fwd
        for k, fn in zip(self.OPS, self.real[1]):
            setattr(self.ops, k, fn)


@pytest.mark.parametrize("num_centroids, with_feature", [(7, True), (7, False), (-1, True), (-1, False)])
def test_set_abstraction_fused_training_within_the_referee_bound(ops, dropin, num_centroids, with_feature):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    torch.manual_seed(20 + num_centroids + with_feature)
    rng = np.random.default_rng(21)
    b, n, c = 2, 48, 4
    sa = modules.SetAbstraction(c if with_feature else 0, (16, 16, 32), num_centroids, 0.3, 8, use_xyz=True).cuda()
    perturb_batchnorm(sa, rng)
    m = n if num_centroids == -1 else num_centroids
    inputs = [dev(dyadic(rng, (b, 3, n))), dev(rng.standard_normal((b, c, n)).astype(np.float32)) if with_feature else None]
    go = dev(rng.standard_normal((b, 32, m)).astype(np.float32))
    with CountedOps(ops) as calls:
        # the float64 and the unfused runs: 3 conv + 3 BatchNorm forwards each; the fused run: none, and no group_points
        referee_module("SetAbstraction M=%d features=%s:" % (num_centroids, with_feature), modules, sa, inputs,
                       [1] if with_feature else [], go,
                       lambda: calls["layers"] == 12 and calls["pn2_sa_rows"] == 1 and calls["pn2_rows_max"] == 1
                       and calls["linear"] == 3 and calls["bn_lrelu"] == 3
                       and calls["group_points"] == 2 * (2 if with_feature else 1))


def test_feature_propagation_fused_training_within_the_referee_bound(ops, dropin):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    torch.manual_seed(30)
    rng = np.random.default_rng(31)
    b, n1, n2 = 2, 48, 12
    fp = modules.FeaturePropagation(8, 4, (16, 16), 3).cuda()
    perturb_batchnorm(fp, rng)
    inputs = [dev(dyadic(rng, (b, 3, n1))), dev(dyadic(rng, (b, 3, n2))),
              dev(rng.standard_normal((b, 4, n1)).astype(np.float32)), dev(rng.standard_normal((b, 8, n2)).astype(np.float32))]
    go = dev(rng.standard_normal((b, 16, n1)).astype(np.float32))
    with CountedOps(ops) as calls:
        referee_module("FeaturePropagation:", modules, fp, inputs, [2, 3], go,
                       lambda: calls["layers"] == 8 and calls["linear"] == 2 and calls["bn_lrelu"] == 2)
    ops.pn2_check_indices()


# ------------------------------------------------------------------------------------------------ the network

def g16_network(dropin, g16, **kw):
    PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    net = PN2SSG(**dict(NET_KW, **kw)).cuda()
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g16.items() if k.startswith("sd/")}, strict=True)
    return net, {"points": dev(g16["points"]), "feature": dev(g16["feature"])}


def test_fused_training_pn2ssg_against_the_reference_classes(ops, dropin, g16, monkeypatch):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
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
    net, batch = g16_network(dropin, g16)
    keys = list(net.state_dict().keys())
    assert pn2ssg.fuse_training(net) is net and list(net.state_dict().keys()) == keys
    net.train()
    with CountedOps(ops) as calls:
        out = net(batch)["seg_logit"]
    # 2 set abstractions x 3 layers, 2 propagations x 2, mlp_seg 1, and the logits' product: no PyTorch layer ran
    assert calls == {"layers": 0, "pn2_sa_rows": 2, "pn2_rows_max": 2, "group_points": 0, "linear": 12, "bn_lrelu": 11}
    for kind, got in seen.items():
        assert len(got) == 2, kind
        for call, index in enumerate(got):
            assert np.array_equal(index, g16["%s_%d" % (kind, call)]), "%s call %d" % (kind, call)
    assert out.shape == g16["logit_train_f32"].shape and out.is_contiguous()
    failures = []
    util.referee_check("g16 PN2SSG fused training logits", host(out), g16["logit_train_f32"], g16["logit_train_f64"],
                       failures=failures)
    out.square().mean().backward()
    names = [n for n, _ in net.named_parameters()]
    assert sorted(names) == sorted(k[len("grad_f64/"):] for k in g16 if k.startswith("grad_f64/"))
    for name, p in net.named_parameters():
        util.referee_check("g16 PN2SSG fused training grad " + name, host(p.grad), g16["grad_f32/" + name],
                           g16["grad_f64/" + name], failures=failures)
    assert not failures, "\n".join(failures)
    assert all(int(b) == 1 for n, b in net.named_buffers() if n.endswith("num_batches_tracked"))
    ops.pn2_check_indices()
    # eval mode is left alone: the PyTorch layers, bit for bit what an unfused network gives
    other, _ = g16_network(dropin, g16)
    other.load_state_dict(net.state_dict())
    with torch.no_grad(), CountedOps(ops) as calls:
        fused_eval, plain_eval = net.eval()(batch)["seg_logit"], other.eval()(batch)["seg_logit"]
    assert calls["layers"] == 2 * 23 and calls["pn2_sa_rows"] == 0 and torch.equal(fused_eval, plain_eval)


def test_fused_training_step_is_bit_reproducible_in_deterministic_mode(ops, dropin, g16, deterministic):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    runs = []
    for _ in range(2):
        net, batch = g16_network(dropin, g16)                    # dropout_prob = 0: no random stream in the step
        modules.fuse_training(net).train()
        feature = batch["feature"].clone().requires_grad_(True)
        out = net({"points": batch["points"], "feature": feature})["seg_logit"]
        out.square().mean().backward()
        res = {"logits": host(out), "grad feature": host(feature.grad)}
        res.update({"grad " + n: host(p.grad) for n, p in net.named_parameters()})
        res.update({n: host(b) for n, b in net.named_buffers()})
        runs.append(res)
    assert sorted(runs[0]) == sorted(runs[1]) and len(runs[0]) > 60
    differ = [k for k in runs[0] if not bits_equal(runs[0][k], runs[1][k])]
    assert not differ, differ
    assert np.abs(runs[0]["grad sa_modules.0.mlp.0.conv.weight"]).max() > 0


def test_fused_set_abstraction_forward_and_backward_in_a_captured_graph(ops, dropin):
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    torch.manual_seed(40)
    rng = np.random.default_rng(41)
    b, n, c = 2, 48, 4
    sa = modules.fuse_training(modules.SetAbstraction(c, (16, 32), 7, 0.3, 8, use_xyz=True).cuda()).train()
    for layer in sa.mlp:
        layer.bn.momentum = 0.0                                  # replays leave the running statistics where they are
    xyz = dev(dyadic(rng, (b, 3, n)))
    feature = dev(rng.standard_normal((b, c, n)).astype(np.float32)).requires_grad_(True)
    go = dev(rng.standard_normal((b, 32, 7)).astype(np.float32))
    params = list(sa.parameters())

    def step():
        out = sa(xyz, feature)[1]
        return (out,) + torch.autograd.grad(out, [feature] + params, go)

    eager = [t.detach().clone() for t in step()]                 # the eager warm-up: the row-count table exists now
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        captured = step()
    for _ in range(2):
        for t in captured:
            t.detach().zero_()
        graph.replay()
        torch.cuda.synchronize()
        for name, got, want in zip(["output", "grad feature"] + [n for n, _ in sa.named_parameters()], captured, eager):
            # the default mode's atomic sums may differ in their last bits from one run to the next: the project's
            # floor for a few float32 roundings (util.REFEREE_FLOOR, relative to the tensor's norm), nothing more
            err = util.l2_err(host(got), host(want))
            assert err <= util.REFEREE_FLOOR, (name, err)
