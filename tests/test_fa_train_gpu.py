"""GPU: the fused FeatureAggregation training path. Operator level: ops.pn2_fa_rows / ops.pn2_rows_sum
(csrc/pn2_rows.hip) against the NumPy restatement of tests/fa_train_ref.py -- forwards and the ordered backward bit for
bit, the atomic backward within (T + 1) u sum|g| -- on a map that is NCHW or channels-last. Module and network level:
FeatureAggregation.forward_rows and MVPNet3D after fuse_training(net, aggregation=True) against the unfused hand-off and
a float64 run of the same modules under util.referee_check, call counts, fall-backs, bit-reproducibility in deterministic
mode and a captured forward + backward. Points lie on multiples of 2^-6, so the point search picks the same indices in
float32 and float64."""
import copy

import numpy as np
import pytest
import torch

import fa_train_ref as ref
import util
from util import bits_equal

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
LAYOUTS = ["nchw", "channels_last"]


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


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


def laid_out(t, layout):
    return t.contiguous(memory_format=torch.channels_last) if layout == "channels_last" else t.contiguous()


def is_laid_out(t, layout):
    return t.is_contiguous(memory_format=torch.channels_last if layout == "channels_last" else torch.contiguous_format)


# ------------------------------------------------------------------------------------------------ aggregation rows

# (B, nv, h, w, C, np, k, use_relation, index). Together: B in {1, 3}, nv in {1, 2}, h x w in {1x1, 6x8}, np in {1, 33, 257}, k
# in {1, 3, 5}: R from 1 to 3 855 (61 tiles of 64 rows, the last a part tile; 16 workgroups of 256). C in {5, 8, 64, 70}: on a
# channels-last map 5 stays on the lane-per-row kernel (below the 8 contiguous channels the tile kernel asks for), 8 and
# 64 are a part and a whole channel tile, 70 two tiles; on an NCHW map 1 and 8 channel groups. index: "random"; "made" =
# random with rows of -1 and an index equal to nv*h*w; "one" = one pixel owns every position.
ROWS_CASES = [(1, 1, 1, 1, 5, 1, 1, True, "random"), (3, 2, 6, 8, 8, 33, 3, True, "random"),
              (1, 2, 6, 8, 64, 257, 5, True, "random"), (3, 1, 6, 8, 70, 257, 3, False, "made"),
              (1, 2, 1, 1, 70, 33, 5, True, "made"), (3, 2, 6, 8, 5, 257, 1, True, "made"),
              (3, 2, 6, 8, 64, 33, 3, True, "one"), (1, 1, 6, 8, 8, 257, 5, False, "random"),
              (3, 2, 6, 8, 70, 257, 5, True, "made")]


def rows_case(b, nv, h, w, c, n, k, kind, seed, coords=dyadic):
    rng = np.random.default_rng(seed)
    p_all = nv * h * w
    fmap, image_xyz, points = dyadic(rng, (b * nv, c, h, w)), coords(rng, (b, nv, h, w, 3)), coords(rng, (b, 3, n))
    if kind == "one":
        index = np.full((b, n, k), p_all - 1, np.int64)
    else:
        index = rng.integers(0, p_all, size=(b, n, k)).astype(np.int64)
    if kind == "made":
        index[rng.random((b, n)) < 0.15] = -1
        index[0, 0] = -1                                         # a row of -1
        index[-1, -1, 0] = p_all                                 # one index past the end
        assert (index == -1).all(axis=2).any() and (index == p_all).any()
    return fmap, image_xyz, points, index


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("b, nv, h, w, c, n, k, use_relation, kind", ROWS_CASES)
def test_rows_forward_and_both_backwards(ops, b, nv, h, w, c, n, k, use_relation, kind, layout):
    fmap, image_xyz, points, index = rows_case(b, nv, h, w, c, n, k, kind, seed=b * 1000 + c * 10 + n + k)
    want = ref.fa_rows(fmap, image_xyz, points, index, use_relation)
    cin, r = want.shape
    assert cin == c + (4 if use_relation else 0) and r == b * n * k
    dx = np.random.default_rng(98).standard_normal((cin, r)).astype(np.float32)
    d_xyz, d_pts, d_idx = dev(image_xyz), dev(points), dev(index)
    results = {}
    for mode in ("atomic", "ordered", "ordered again"):
        ops.set_deterministic(mode != "atomic")
        try:
            ft = laid_out(dev(fmap), layout).requires_grad_(True)
            assert is_laid_out(ft, layout)
            x = ops.pn2_fa_rows(ft, d_xyz, d_pts, d_idx, use_relation=use_relation)
            assert x.shape == (cin, r) and x.is_contiguous()
            assert bits_equal(host(x), want)                     # a gather, rounded differences, a rounded squared distance
            x.backward(dev(dx))
            assert ft.grad.shape == ft.shape and is_laid_out(ft.grad, layout)       # the map's own memory format
            results[mode] = host(ft.grad)
        finally:
            ops.set_deterministic(False)
    wide, scale, count = ref.fa_rows_bwd_wide(dx, index, c, nv, h, w)
    err = np.abs(results["atomic"].astype(np.float64) - wide)
    bound = (count + 1) * U32 * scale                            # T rounded additions in any order
    print("pn2_fa_rows atomic bwd %s %s: max err / bound %.3f, most contributions %d"
          % ((b, nv, h, w, c, n, k, kind), layout, float((err / np.maximum(bound, 1e-300)).max()), int(count.max())))
    assert np.all(err <= bound)
    empty = np.broadcast_to(count == 0, err.shape)
    oracle = ref.fa_rows_bwd(dx, index, c, nv, h, w)
    for mode in ("ordered", "ordered again"):
        assert bits_equal(results[mode], oracle), mode          # acc = fl(acc + g) over ascending positions
        assert not np.signbit(results[mode][empty]).any() and np.all(results[mode][empty] == 0)
    assert np.all(results["atomic"][empty] == 0)
    assert kind != "one" or (empty.any() and count.max() == n * k)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_relation_is_rounded_operation_by_operation(ops, layout):
    """Coordinates that are NOT dyadic: a fused multiply-add in the squared distance, or another order of its sum, would
    change the last bit of some row."""
    b, nv, h, w, c, n, k = 2, 2, 6, 8, 8, 300, 3
    fmap, image_xyz, points, index = rows_case(b, nv, h, w, c, n, k, "made", seed=77,
                                               coords=lambda rng, shape: rng.standard_normal(shape).astype(np.float32))
    want = ref.fa_rows(fmap, image_xyz, points, index, True)
    d64 = want[c:c + 3].astype(np.float64)
    assert ((d64 ** 2).sum(0).astype(np.float32) != want[c + 3]).any()              # the order and the roundings matter here
    with torch.no_grad():
        x = ops.pn2_fa_rows(laid_out(dev(fmap), layout), dev(image_xyz), dev(points), dev(index))
    assert bits_equal(host(x), want)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_rows_ordered_backward_walks_a_pixel_with_1536_entries(ops, deterministic, layout):
    b, nv, h, w, c, n, k = 1, 2, 6, 8, 8, 512, 3                 # one pixel with np*k = 1 536 entries
    rng = np.random.default_rng(3)
    fmap, image_xyz, points = dyadic(rng, (b * nv, c, h, w)), dyadic(rng, (b, nv, h, w, 3)), dyadic(rng, (b, 3, n))
    index = np.full((b, n, k), 59, np.int64)                     # view 1, row 1, column 3
    dx = rng.standard_normal((c + 4, b * n * k)).astype(np.float32)
    ft = laid_out(dev(fmap), layout).requires_grad_(True)
    ops.pn2_fa_rows(ft, dev(image_xyz), dev(points), dev(index)).backward(dev(dx))
    got, want = host(ft.grad), ref.fa_rows_bwd(dx, index, c, nv, h, w)
    assert bits_equal(got, want)
    assert np.all(got[1, :, 1, 3] != 0) and np.count_nonzero(got) == c and not np.signbit(got[got == 0]).any()
    # the order matters on this pixel: the sum of the same values in descending order is another float
    assert not np.array_equal(want[1, :, 1, 3], ref.fa_rows_bwd(dx[:, ::-1].copy(), index, c, nv, h, w)[1, :, 1, 3])


def test_rows_and_group_points_share_one_csr(ops, deterministic, monkeypatch):
    rng = np.random.default_rng(8)
    b, nv, h, w, c, n, k = 2, 2, 6, 8, 4, 40, 3
    p_all = nv * h * w
    index = dev(rng.integers(0, p_all, size=(b, n, k)).astype(np.int64))
    built = []
    real = ops.index_csr
    monkeypatch.setattr(ops, "index_csr", lambda *a, **kw: built.append(1) or real(*a, **kw))
    f1 = dev(rng.standard_normal((b * nv, c, h, w)).astype(np.float32)).requires_grad_(True)
    f2 = dev(rng.standard_normal((b, c, p_all)).astype(np.float32)).requires_grad_(True)
    image_xyz, points = dev(dyadic(rng, (b, nv, h, w, 3))), dev(dyadic(rng, (b, 3, n)))
    assert ops.index_csr_for(index, p_all) is None
    ops.pn2_fa_rows(f1, image_xyz, points, index).sum().backward()
    csr = ops.index_csr_for(index, p_all)
    assert csr is not None and len(built) == 1
    ops.group_points(f2, index).sum().backward()
    assert len(built) == 1 and ops.index_csr_for(index, p_all)[0] is csr[0] and ops.index_csr_for(index, p_all)[1] is csr[1]
    ops.pn2_fa_rows(f1, image_xyz, points, index).sum().backward()
    assert len(built) == 1
    # the same sums from both ops (two backwards of the rows, one of group_points): counts, exact in float32
    assert np.array_equal(ref.pixel_planes(host(f1.grad), b), 2 * host(f2.grad)) and host(f2.grad).max() >= 2


def test_rows_refuse_coordinates_that_require_a_gradient(ops):
    fmap = torch.zeros(2, 4, 2, 3, device="cuda")
    image_xyz, points = torch.zeros(1, 2, 2, 3, 3, device="cuda"), torch.zeros(1, 3, 5, device="cuda")
    index = torch.zeros(1, 5, 3, dtype=torch.int64, device="cuda")
    with pytest.raises(RuntimeError, match="no gradient for coordinates"):
        ops.pn2_fa_rows(fmap, image_xyz.clone().requires_grad_(True), points, index)
    with pytest.raises(RuntimeError, match="no gradient for coordinates"):
        ops.pn2_fa_rows(fmap, image_xyz, points.clone().requires_grad_(True), index)
    with pytest.raises(RuntimeError, match="holds 1 images"):
        ops.pn2_fa_rows(fmap[:1], image_xyz, points, index)
    with torch.no_grad():
        assert ops.pn2_fa_rows(fmap, image_xyz, points.clone().requires_grad_(True), index).shape == (8, 15)


class LibrarySpy(object):
    """Stands in for ops.lib(): records the names of the aggregation backward entry points that are fetched."""

    def __init__(self, lib):
        self._lib, self.fetched = lib, []

    def __getattr__(self, name):
        if name.startswith("mvk_pn2_fa_rows_bwd"):
            self.fetched.append(name)
        return getattr(self._lib, name)


@pytest.mark.parametrize("det", [False, True])
def test_rows_backward_launches_nothing_for_a_map_without_gradient(ops, monkeypatch, det):
    rng = np.random.default_rng(4)
    b, nv, h, w, c, n, k = 2, 2, 6, 8, 8, 20, 3
    fmap, image_xyz, points, index = rows_case(b, nv, h, w, c, n, k, "random", seed=5)
    spy = LibrarySpy(ops.lib())
    monkeypatch.setattr(ops, "lib", lambda: spy)
    weight = dev(rng.standard_normal((6, c + 4)).astype(np.float32)).requires_grad_(True)
    ops.set_deterministic(det)
    try:
        for needs in (False, True):
            ft = dev(fmap).requires_grad_(needs)
            x = ops.pn2_fa_rows(ft, dev(image_xyz), dev(points), dev(index))
            assert x.requires_grad == needs
            (weight @ x).sum().backward()
            assert (ft.grad is not None) == needs
            assert spy.fetched == (["mvk_pn2_fa_rows_bwd_csr" if det else "mvk_pn2_fa_rows_bwd"] if needs else [])
    finally:
        ops.set_deterministic(False)
    assert weight.grad is not None


# ------------------------------------------------------------------------------------------------ sum over the neighbours

# (B, M, K, Cout): Cout in {5, 64, 130} (a part tile, one tile, two tiles and a part), K in {1, 3, 5, 33}, M in {1, 31, 65}
# (a part tile, two tiles and a part), B in {1, 3}
SUM_CASES = [(1, 1, 1, 5), (3, 31, 3, 64), (1, 65, 5, 130), (3, 65, 33, 5), (1, 31, 33, 130), (3, 1, 5, 64), (3, 65, 3, 130)]


@pytest.mark.parametrize("b, m, k, cout", SUM_CASES)
def test_rows_sum_forward_and_backward_are_exact(ops, b, m, k, cout):
    rng = np.random.default_rng(b * 100 + m + k + cout)
    y = rng.standard_normal((b * m * k, cout)).astype(np.float32)
    want = ref.rows_sum(y, b, m, k)
    yt = dev(y).requires_grad_(True)
    out = ops.pn2_rows_sum(yt, b, m, k)
    assert out.shape == (b, cout, m) and out.is_contiguous()
    assert bits_equal(host(out), want)                           # ascending k, one rounding per addition
    if k >= 5:                                                   # ... which another order of the same rows does not give
        assert not np.array_equal(want, ref.rows_sum(y.reshape(b, m, k, cout)[:, :, ::-1].reshape(y.shape), b, m, k))
    g = rng.standard_normal((b, cout, m)).astype(np.float32)
    out.backward(dev(g))
    assert bits_equal(host(yt.grad), ref.rows_sum_bwd(g, k))     # g in each of the k rows
    assert torch.equal(ops.pn2_rows_sum(yt.detach(), b, m, k), out.detach())


def test_rows_sum_treats_negative_zero_and_nan_as_float32_addition_does(ops):
    rng = np.random.default_rng(12)
    b, m, k, cout = 2, 3, 5, 70
    y = rng.standard_normal((b * m * k, cout)).astype(np.float32)
    y[0:5, 0] = -0.0                                             # group (0, 0): every row -0 -> -0
    y[5:10, 0] = -0.0
    y[7, 0] = 0.0                                                # group (0, 1): one +0 among -0 -> +0
    y[11, 3] = y[13, 3] = np.nan                                 # group (0, 2)
    y[29, 69] = np.nan                                           # the last row of the last group
    y[15:20, 1] = [np.inf, 1, -np.inf, 2, 3]                     # group (1, 0): inf - inf
    with np.errstate(invalid="ignore"):
        want = ref.rows_sum(y, b, m, k)
    got = host(ops.pn2_rows_sum(dev(y), b, m, k))
    nan = np.isnan(want)
    assert nan.sum() == 3 and nan[0, 3, 2] and nan[1, 69, 2] and nan[1, 1, 0] and np.array_equal(np.isnan(got), nan)
    assert bits_equal(got[~nan], want[~nan])
    assert got[0, 0, 0] == 0 and np.signbit(got[0, 0, 0]) and got[0, 0, 1] == 0 and not np.signbit(got[0, 0, 1])
    one = host(ops.pn2_rows_sum(dev(np.full((3, 2), -0.0, np.float32)), 1, 3, 1))   # K = 1: a copy
    assert np.signbit(one).all()


# ------------------------------------------------------------------------------------------------ the module

SMALL = dict(b=3, nv=2, h=6, w=8, c=8, n=128, k=3)               # small_mvpnet's sizes (test_pn2_fa_gpu.py)


def perturb_batchnorm(net, rng):
    with torch.no_grad():
        for mod in net.modules():
            if isinstance(mod, torch.nn.modules.batchnorm._BatchNorm):
                for t, v in ((mod.weight, 1 + 0.1 * rng.standard_normal(mod.weight.shape)),
                             (mod.bias, 0.1 * rng.standard_normal(mod.bias.shape)),
                             (mod.running_mean, 0.1 * rng.standard_normal(mod.bias.shape)),
                             (mod.running_var, 1 + 0.1 * np.abs(rng.standard_normal(mod.bias.shape)))):
                    t.copy_(torch.from_numpy(v).float())


def handoff(ops, fa, fmap, image_xyz, index, points):
    """MVPNet3D.forward's own steps from the encoder's map to the aggregated features."""
    b, nv, h, w, _ = image_xyz.shape
    f = fmap.reshape(b, nv, -1, h, w).transpose(1, 2).contiguous().reshape(b, -1, nv * h * w)
    f = ops.group_points(f, index)
    with torch.no_grad():
        xyz = ops.group_points(image_xyz.permute(0, 4, 1, 2, 3).reshape(b, 3, nv * h * w), index)
    return fa(xyz, points, f)


def run_aggregation(ops, fa, tensors, go, dtype, fused):
    """One training forward + backward of a copy of `fa` in `dtype`: output, map gradient, parameter gradients, running
    statistics and batch counters, all on the host."""
    mod = copy.deepcopy(fa).to(dtype).train()
    mod._fused_training = fused
    fmap, image_xyz, index, points = [(t.to(dtype) if t.is_floating_point() else t).clone() for t in tensors]
    assert fmap.stride() == tensors[0].stride()
    fmap.requires_grad_(True)
    assert mod._use_rows(fmap, image_xyz, points) == fused
    out = mod.forward_rows(fmap, image_xyz, index, points) if fused else handoff(ops, mod, fmap, image_xyz, index, points)
    out.backward(go.to(dtype))
    res = {"output": host(out), "grad map": host(fmap.grad)}
    assert not fused or fmap.grad.stride() == fmap.stride()
    for name, p in mod.named_parameters():
        res["grad " + name] = host(p.grad)
    counters = {}
    for name, buf in mod.named_buffers():
        if name.endswith("num_batches_tracked"):
            counters[name] = int(buf)
        else:
            res[name] = host(buf)
    return res, counters


class CountedOps(object):
    """Counts the calls of the ops of the fused training path and the forwards of the PyTorch layers it replaces."""
    LAYERS = (torch.nn.Conv1d, torch.nn.Conv2d, torch.nn.BatchNorm1d, torch.nn.BatchNorm2d)
    OPS = ("pn2_fa_rows", "pn2_rows_sum", "pn2_rows_max", "pn2_sa_rows", "group_points", "linear", "bn_lrelu")

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


def aggregation_inputs(rng, c, layout, s=SMALL):
    b, nv, h, w, n, k = s["b"], s["nv"], s["h"], s["w"], s["n"], s["k"]
    fmap = laid_out(dev(rng.standard_normal((b * nv, c, h, w)).astype(np.float32)), layout)
    return [fmap, dev(rng.random((b, nv, h, w, 3)).astype(np.float32)),
            dev(rng.integers(0, nv * h * w, size=(b, n, k)).astype(np.int64)), dev(dyadic(rng, (b, 3, n)))]


@pytest.mark.parametrize("c, widths, reduction, use_relation, layout", [
    (8, (8, 8), "sum", True, "nchw"), (8, (8, 8), "max", True, "channels_last"),
    (8, (8, 8), "sum", False, "channels_last"), (8, (8, 8), "max", False, "nchw"),
    (64, (64, 64, 64), "sum", True, "channels_last"), (64, (64, 64, 64), "max", True, "nchw"),
    (64, (64, 64, 64), "sum", False, "nchw"), (64, (64, 64, 64), "max", False, "channels_last")])
def test_aggregation_rows_within_the_referee_bound(ops, dropin, c, widths, reduction, use_relation, layout):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    torch.manual_seed(50 + c + len(reduction) + use_relation)
    rng = np.random.default_rng(51)
    fa = m3.FeatureAggregation(c, widths, reduction=reduction, use_relation=use_relation).cuda()
    perturb_batchnorm(fa, rng)
    tensors = aggregation_inputs(rng, c, layout)
    go = dev(rng.standard_normal((SMALL["b"], widths[-1], SMALL["n"])).astype(np.float32))
    with CountedOps(ops) as calls:
        f64, n64 = run_aggregation(ops, fa, tensors, go, torch.float64, False)
        unfused, n32 = run_aggregation(ops, fa, tensors, go, torch.float32, False)
        before = dict(calls)
        fused, nf = run_aggregation(ops, fa, tensors, go, torch.float32, True)
    # the float64 and the unfused runs: a Conv2d and a BatchNorm2d forward per layer and two group_points each; the fused
    # run: none of them
    assert before["layers"] == calls["layers"] == 4 * len(widths) and before["group_points"] == calls["group_points"] == 4
    assert before["pn2_fa_rows"] == 0 and calls["pn2_fa_rows"] == 1 and calls["linear"] == calls["bn_lrelu"] == len(widths)
    assert (calls["pn2_rows_sum"], calls["pn2_rows_max"]) == ((1, 0) if reduction == "sum" else (0, 1))
    assert sorted(fused) == sorted(unfused) == sorted(f64) and nf == n32 == n64 and all(v == 1 for v in nf.values())
    assert len(nf) == len(widths) and sum(k.endswith("running_var") for k in fused) == len(widths)
    assert sum(k.startswith("grad mlp.") for k in fused) == 3 * len(widths) and "grad map" in fused
    failures = []
    label = "FeatureAggregation(%d, %s) %s relation=%s %s:" % (c, widths, reduction, use_relation, layout)
    for key in sorted(fused):
        assert fused[key].shape == f64[key].shape and fused[key].dtype == np.float32
        util.referee_check("%s %s" % (label, key), fused[key], unfused[key], f64[key], failures=failures)
    assert not failures, "\n".join(failures)
    assert np.abs(fused["grad map"]).max() > 0


# ------------------------------------------------------------------------------------------------ the network

class MapEncoder(torch.nn.Module):
    """Stands for the 2D encoder: returns a stored map, NCHW or channels-last, whatever the images are. Nothing of
    MIOpen is in the picture, and the map's gradient is a leaf's .grad."""

    def __init__(self, fmap):
        super().__init__()
        self.map = torch.nn.Parameter(fmap)

    def forward(self, data):
        return {"feature": self.map}


def small_network(dropin, layout, reduction="sum", s=SMALL):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    torch.manual_seed(3)
    rng = np.random.default_rng(19)
    b, nv, h, w, c, n, k = s["b"], s["nv"], s["h"], s["w"], s["c"], s["n"], s["k"]
    net_3d = pn2ssg.PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    fmap = laid_out(torch.from_numpy(rng.standard_normal((b * nv, c, h, w)).astype(np.float32)).cuda(), layout)
    net = m3.MVPNet3D(MapEncoder(fmap), None, net_3d, in_channels=c, mlp_channels=(8, 8), reduction=reduction,
                      use_relation=True).cuda().train()
    assert is_laid_out(net.net_2d.map, layout) and net.net_2d.map.stride() == fmap.stride()
    perturb_batchnorm(net, np.random.default_rng(18))
    batch = {"images": torch.zeros(b, nv, 3, h, w).cuda(), "image_xyz": dev(rng.random((b, nv, h, w, 3)).astype(np.float32)),
             "knn_indices": dev(rng.integers(0, nv * h * w, size=(b, n, k)).astype(np.int64)),
             "points": dev(dyadic(rng, (b, 3, n)))}
    return net, batch, pn2ssg


def network_step(net, batch, dtype=torch.float32):
    """Forward + backward of a copy of `net` in `dtype` and training mode: logits, every gradient (the map's is the
    encoder parameter's), every buffer."""
    net = copy.deepcopy(net).to(dtype).train()
    out = net({key: (v.to(dtype) if v.is_floating_point() else v) for key, v in batch.items()})["seg_logit"]
    out.square().mean().backward()
    res = {"logits": host(out)}
    res.update({"grad " + n: host(p.grad) for n, p in net.named_parameters()})
    res.update({n: host(b) for n, b in net.named_buffers()})
    assert net.net_2d.map.grad.shape == net.net_2d.map.shape
    return res


@pytest.mark.parametrize("layout, reduction", [("nchw", "sum"), ("channels_last", "max")])
def test_fused_training_mvpnet_against_the_float64_network(ops, dropin, layout, reduction):
    net, batch, pn2ssg = small_network(dropin, layout, reduction)
    keys = list(net.state_dict().keys())
    f64 = network_step(net, batch, torch.float64)
    with CountedOps(ops) as calls:
        unfused = network_step(net, batch)
    assert calls["pn2_fa_rows"] == 0 and calls["group_points"] >= 2 and calls["layers"] > 5
    fused_net = pn2ssg.fuse_training(copy.deepcopy(net), aggregation=True)
    assert fused_net.feat_aggreg._fused_training and list(fused_net.state_dict().keys()) == keys
    with CountedOps(ops) as calls:
        fused = network_step(fused_net, batch)
    # aggregation 2 layers, set abstraction 2, propagation 1, mlp_seg 1, and the logits' product; the reduction of the
    # aggregation, and the set abstraction's max: no PyTorch layer and no group_points ran
    n_max = 1 + (reduction == "max")
    assert calls == {"layers": 0, "pn2_fa_rows": 1, "pn2_rows_sum": 2 - n_max, "pn2_rows_max": n_max, "pn2_sa_rows": 1,
                     "group_points": 0, "linear": 7, "bn_lrelu": 6}
    ops.pn2_check_indices()
    assert sorted(fused) == sorted(unfused) == sorted(f64) and "grad net_2d.map" in fused
    failures = []
    for key in sorted(fused):
        if key.endswith("num_batches_tracked"):
            assert fused[key] == unfused[key] == f64[key] == 1, key
            continue
        util.referee_check("MVPNet3D fused training (%s, %s) %s" % (layout, reduction, key), fused[key], unfused[key],
                           f64[key], failures=failures)
    assert not failures, "\n".join(failures)
    assert np.abs(fused["grad net_2d.map"]).max() > 0


def test_lengths_eval_mode_and_unfuse_leave_the_aggregation_as_it_was(ops, dropin):
    net, batch, pn2ssg = small_network(dropin, "channels_last")
    fused_net = pn2ssg.fuse_training(copy.deepcopy(net), aggregation=True)

    def logits(model, data, train, eval_3d=False):
        model = copy.deepcopy(model).train(train)
        if eval_3d:
            model.net_3d.eval()
        with torch.no_grad(), CountedOps(ops) as calls:
            return model(data)["seg_logit"], calls

    # a padded batch with the aggregation in training mode (PN2SSG takes `lengths` in eval mode only): BatchNorm over
    # padded rows would be another function, so the hand-off is the unfused one
    padded = dict(batch, lengths=dev(np.asarray([128, 91, 32], np.int64)))
    got, calls = logits(fused_net, padded, True, eval_3d=True)
    assert calls["pn2_fa_rows"] == 0 and calls["group_points"] >= 2
    assert torch.equal(got, logits(net, padded, True, eval_3d=True)[0])
    got, calls = logits(fused_net, batch, True, eval_3d=True)       # ... and without `lengths` the same model takes the rows
    assert calls["pn2_fa_rows"] == 1
    # eval mode
    got, calls = logits(fused_net, batch, False)
    assert calls["pn2_fa_rows"] == calls["pn2_sa_rows"] == 0 and torch.equal(got, logits(net, batch, False)[0])
    # the one-argument call: the 3D network runs on its rows, the hand-off is the unfused one
    fused_3d = pn2ssg.fuse_training(copy.deepcopy(net))
    assert not fused_3d.feat_aggreg._fused_training
    got, calls = logits(fused_3d, batch, True)
    assert calls["pn2_fa_rows"] == 0 and calls["pn2_sa_rows"] == 1 and calls["group_points"] == 2
    got, calls = logits(fused_net, batch, True)
    assert calls["pn2_fa_rows"] == 1 and calls["group_points"] == 0
    pn2ssg.unfuse_training(fused_net)
    assert not fused_net.feat_aggreg._fused_training and not fused_net.net_3d._fused_training
    got, calls = logits(fused_net, batch, True)
    assert calls["pn2_fa_rows"] == calls["pn2_sa_rows"] == 0 and torch.equal(got, logits(net, batch, True)[0])
    # float64 and a module without an MLP never take the rows
    fused_net = pn2ssg.fuse_training(fused_net, aggregation=True)
    batch64 = {key: (v.double() if v.is_floating_point() else v) for key, v in batch.items()}
    got, calls = logits(copy.deepcopy(fused_net).double(), batch64, True)
    assert calls["pn2_fa_rows"] == 0 and got.dtype == torch.float64


@pytest.mark.parametrize("layout", LAYOUTS)
def test_fused_mvpnet_step_is_bit_reproducible_in_deterministic_mode(ops, dropin, deterministic, layout):
    net, batch, pn2ssg = small_network(dropin, layout)
    pn2ssg.fuse_training(net, aggregation=True)
    runs = [network_step(net, batch) for _ in range(2)]          # dropout_prob = 0: no random stream in the step
    assert sorted(runs[0]) == sorted(runs[1]) and len(runs[0]) == 40   # logits, 21 gradients (the map's too), 18 buffers
    differ = [k for k in runs[0] if not bits_equal(runs[0][k], runs[1][k])]
    assert not differ, differ
    assert np.abs(runs[0]["grad net_2d.map"]).max() > 0 and np.abs(runs[0]["grad feat_aggreg.mlp.0.conv.weight"]).max() > 0


@pytest.mark.parametrize("det", [False, True])
def test_fused_aggregation_forward_and_backward_in_a_captured_graph(ops, dropin, det):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    torch.manual_seed(40)
    rng = np.random.default_rng(41)
    fa = modules.fuse_training(m3.FeatureAggregation(8, (8, 16)).cuda(), aggregation=True).train()
    for layer in fa.mlp:
        layer.bn.momentum = 0.0                                  # replays leave the running statistics where they are
    fmap, image_xyz, index, points = aggregation_inputs(rng, 8, "channels_last")
    fmap.requires_grad_(True)
    go = dev(rng.standard_normal((SMALL["b"], 16, SMALL["n"])).astype(np.float32))
    params = list(fa.parameters())

    def step():
        out = fa.forward_rows(fmap, image_xyz, index, points)
        return (out,) + torch.autograd.grad(out, [fmap] + params, go)

    ops.set_deterministic(det)
    try:
        eager = [t.detach().clone() for t in step()]             # the eager warm-up: the row-count table and the CSR exist now
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
            for name, got, want in zip(["output", "grad map"] + [n for n, _ in fa.named_parameters()], captured, eager):
                if det:
                    assert bits_equal(host(got), host(want)), name
                else:
                    # the default mode's atomic sums may differ in their last bits from one run to the next: the project's
                    # floor for a few float32 roundings (util.REFEREE_FLOOR, relative to the tensor's norm), nothing more
                    err = util.l2_err(host(got), host(want))
                    assert err <= util.REFEREE_FLOOR, (name, err)
    finally:
        ops.set_deterministic(False)
