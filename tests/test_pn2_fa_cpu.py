"""CPU-only: the host side of the fused frozen FeatureAggregation (pn2_fa_k of csrc/pn2_mlp.hip, ops.pn2_fa_mlp,
freeze_inference(net, aggregation=True)): the export, the wrapper's refusals, the NumPy restatement of
tests/pn2_fa_ref.py against FeatureAggregation.forward in torch float64, and the snapshot's life cycle and fold."""
import ctypes

import numpy as np
import pytest
import torch

import pn2_fa_ref as ref
import pn2_frozen_ref as fref


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def mods():
    import mvkpconv
    return (mvkpconv.sub("dropin.mvpnet.models.mvpnet_3d"), mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg"),
            mvkpconv.sub("dropin.mvpnet.models.pn2.modules"))


def test_library_exports_the_aggregation_entry_point_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    name = "mvk_pn2_fa_fwd"
    assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9


def fa_args(b=2, nv=2, c=3, h=3, w=5, n=6, k=3, widths=(7, 6)):
    params = torch.zeros(sum(widths[i + 1] * (widths[i] + 1) for i in range(len(widths) - 1)))
    return [torch.zeros(b * nv, c, h, w), torch.zeros(b, nv, h, w, 3), torch.zeros(b, 3, n),
            torch.zeros(b, n, k, dtype=torch.int64), params, widths]


def test_wrapper_refuses_what_it_does_not_run(ops):
    fn = ops.pn2_fa_mlp
    with pytest.raises(RuntimeError, match="HBM"):              # CPU tensors, like the other pn2 wrappers
        fn(*fa_args())
    for pos in (0, 1, 2, 4):                                    # a float64 operand, the packed parameters included
        a = fa_args()
        a[pos] = a[pos].double()
        with pytest.raises(RuntimeError, match="float32"):
            fn(*a)
    a = fa_args()
    a[2] = torch.zeros(2, 6, 3).transpose(1, 2)                 # (2,3,6) values, not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        fn(*a)
    a = fa_args()
    a[0] = torch.zeros(4, 3, 3, 10)[:, :, :, ::2]               # the right shape, neither contiguous nor channels-last
    with pytest.raises(RuntimeError, match="contiguous or channels-last"):
        fn(*a)
    a = fa_args()
    a[0] = a[0].contiguous(memory_format=torch.channels_last)   # a channels-last map gets as far as the device check
    assert not a[0].is_contiguous()
    with pytest.raises(RuntimeError, match="HBM"):
        fn(*a)
    a = fa_args()
    a[3] = a[3].int()
    with pytest.raises(RuntimeError, match="int64"):
        fn(*a)
    for pos in (0, 4):
        a = fa_args()
        a[pos].requires_grad_(True)
        with pytest.raises(RuntimeError, match="no backward"):
            fn(*a)
        with torch.no_grad():                                   # with gradients off the same call gets as far as the device check
            with pytest.raises(RuntimeError, match="HBM"):
                fn(*a)


def test_wrapper_refuses_bad_shapes_and_options(ops):
    fn = ops.pn2_fa_mlp
    a = fa_args()
    a[0] = torch.zeros(5, 3, 3, 5)                              # B * nv = 4 images expected
    with pytest.raises(RuntimeError, match="holds 5 images"):
        fn(*a)
    a = fa_args()
    a[0] = torch.zeros(4, 3, 5, 3)                              # h x w differs from image_xyz's
    with pytest.raises(RuntimeError, match="expected feature_2d"):
        fn(*a)
    a = fa_args()
    a[3] = torch.zeros(2, 7, 3, dtype=torch.int64)              # N differs from the points'
    with pytest.raises(RuntimeError, match="expected feature_2d"):
        fn(*a)
    with pytest.raises(RuntimeError, match=r"widths\[0\] = 7, the input rows hold 3"):
        fn(*fa_args(), use_relation=False)
    with pytest.raises(RuntimeError, match=r"widths\[0\] = 3, the input rows hold 7"):
        fn(*fa_args(widths=(3, 6)))
    with pytest.raises(RuntimeError, match="reduction"):
        fn(*fa_args(), reduction="mean")
    with pytest.raises(RuntimeError, match="lengths must be an int64"):
        fn(*fa_args(), lengths=torch.zeros(2, dtype=torch.int32))
    with pytest.raises(RuntimeError, match="lengths must have shape"):
        fn(*fa_args(), lengths=torch.zeros(3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HBM"):
        fn(*fa_args(), lengths=torch.zeros(2, dtype=torch.int64))


def perturb(net, rng, dtype=torch.float64):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                for t, v in ((m.weight, 1 + 0.1 * rng.standard_normal(m.weight.shape)), (m.bias, 0.1 * rng.standard_normal(m.bias.shape)),
                             (m.running_mean, 0.1 * rng.standard_normal(m.bias.shape)),
                             (m.running_var, 1 + 0.1 * np.abs(rng.standard_normal(m.bias.shape)))):
                    t.copy_(torch.from_numpy(v).to(t.dtype))


@pytest.mark.parametrize("reduction", ["sum", "max"])
@pytest.mark.parametrize("use_relation", [True, False])
def test_restatement_agrees_with_feature_aggregation_in_float64(mods, reduction, use_relation):
    rng = np.random.default_rng(7)
    b, nv, c, h, w, n, k = 2, 2, 3, 3, 5, 9, 4
    p = nv * h * w
    fa = mods[0].FeatureAggregation(c, mlp_channels=(6, 7), reduction=reduction, use_relation=use_relation).double().eval()
    perturb(fa, rng)
    fmap = rng.standard_normal((b * nv, c, h, w))
    image_xyz, points = rng.random((b, nv, h, w, 3)), rng.random((b, 3, n))
    index = rng.integers(0, p, size=(b, n, k))
    index[0, 1, 2:] = -1                                        # a tail, a whole point and an index past the pixels
    index[1, 3] = -1
    index[1, 5, 0] = p + 3
    sd = {"mlp." + key: v.numpy() for key, v in fa.mlp.state_dict().items()}
    params, widths = fref.fold_stack(sd, "mlp", 2, dtype=np.float64)
    assert widths == (c + (4 if use_relation else 0), 6, 7)
    got = ref.fa_mlp(fmap, image_xyz, points, index, params, widths, reduction=reduction, use_relation=use_relation)

    def grouped(t):                                             # (b,C,P) -> (b,C,n,k), zero where the index is outside
        idx = torch.from_numpy(index)
        ok = (idx >= 0) & (idx < p)
        flat = torch.where(ok, idx, torch.zeros_like(idx)).reshape(b, 1, n * k).expand(-1, t.shape[1], -1)
        return torch.gather(t, 2, flat).reshape(b, -1, n, k) * ok.unsqueeze(1)

    with torch.no_grad():                                       # MVPNet3D.forward's own reshapes, then forward()
        f = torch.from_numpy(fmap).reshape(b, nv, c, h, w).transpose(1, 2).reshape(b, c, p)
        x = torch.from_numpy(image_xyz).permute(0, 4, 1, 2, 3).reshape(b, 3, p)
        want = fa(grouped(x), torch.from_numpy(points), grouped(f)).numpy()
    assert got.shape == want.shape == (b, 7, n)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    # columns behind lengths are zeros whatever they hold; the others do not move
    points[1, :, 4:] = np.nan
    index[1, 4:] = 1 << 40
    cut = ref.fa_mlp(fmap, image_xyz, points, index, params, widths, reduction=reduction, use_relation=use_relation,
                     lengths=[n + 5, 4])
    assert np.array_equal(cut[0], got[0]) and np.array_equal(cut[1, :, :4], got[1, :, :4]) and not cut[1, :, 4:].any()


class StandIn2D(torch.nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def small_mvpnet(mods, **kw):
    torch.manual_seed(4)
    net_3d = mods[1].PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                            fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = mods[0].MVPNet3D(StandIn2D(8), None, net_3d, **dict(dict(in_channels=8, mlp_channels=(8, 8), reduction="sum",
                                                                   use_relation=True), **kw)).eval()
    perturb(net, np.random.default_rng(17))
    return net


def test_snapshot_is_taken_on_request_only_and_dropped_by_train_and_unfreeze(mods):
    m3, pn2ssg, modules = mods
    net = small_mvpnet(mods)
    fa = net.feat_aggreg
    keys = list(net.state_dict().keys())
    assert fa._frozen is None
    assert modules.freeze_inference(net) is net                 # the one-argument call leaves the aggregation alone
    assert fa._frozen is None and net.net_3d.sa_modules[0]._frozen is not None
    assert pn2ssg.freeze_inference(net, aggregation=True) is net
    params, widths, reduction, use_relation = fa._frozen
    assert widths == (12, 8, 8) and reduction == "sum" and use_relation is True
    assert params.dtype == torch.float32 and params.is_contiguous() and list(net.state_dict().keys()) == keys
    # the fold against a float64 NumPy fold of the same state dict
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    want, want_widths = fref.fold_stack(sd, "feat_aggreg.mlp", 2)
    assert want_widths == widths and params.numpy().shape == want.shape
    assert np.abs(sd["feat_aggreg.mlp.0.bn.running_mean"]).max() > 0.01
    assert np.all(np.abs(params.numpy().astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want))
    # a plain freeze afterwards keeps the aggregation's snapshot; train(True) on the module drops it, eval() does not
    modules.freeze_inference(net)
    assert fa._frozen is not None
    net.eval()
    assert fa._frozen is not None
    fa.train()
    assert fa._frozen is None and net.net_3d.sa_modules[0]._frozen is not None
    modules.freeze_inference(net.eval(), aggregation=True)
    net.train()
    assert fa._frozen is None and net.net_3d._frozen is None
    modules.freeze_inference(net.eval(), aggregation=True)
    assert fa._frozen is not None and modules.unfreeze_inference(net) is net and fa._frozen is None
    assert list(net.state_dict().keys()) == keys


def test_aggregations_the_kernel_does_not_cover_are_left_alone(mods):
    FeatureAggregation, freeze = mods[0].FeatureAggregation, mods[2].freeze_inference
    for kw in (dict(mlp_channels=()), dict(mlp_channels=(8, 8, 8, 8)), dict(mlp_channels=(8, 600))):
        fa = FeatureAggregation(8, reduction="sum", **kw).eval()
        assert freeze(fa, aggregation=True) is fa and fa._frozen is None, kw    # no MLP, four layers, a layer above 512
    fa = FeatureAggregation(8, mlp_channels=(9,), reduction="max", use_relation=False).eval()
    assert freeze(fa, aggregation=True)._frozen[1:] == ((8, 9), "max", False)
    assert freeze(FeatureAggregation(8).eval(), aggregation=True)._frozen[1:] == ((12, 64, 64, 64), "sum", True)
