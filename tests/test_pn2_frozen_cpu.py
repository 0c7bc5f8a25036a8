"""CPU-only: the host side of the frozen PointNet++ inference path (csrc/pn2_mlp.hip, ops.pn2_sa_mlp_max / pn2_fp_mlp,
freeze_inference of dropin/mvpnet/models/pn2): exports, refusals, the BatchNorm fold against a float64 NumPy fold of the
same state dict, and the NumPy restatement of tests/pn2_frozen_ref.py against a plain torch float64 SharedMLP + max."""
import ctypes

import numpy as np
import pytest
import torch

import pn2_frozen_ref as ref

NET_KW = dict(in_channels=4, num_classes=5, sa_channels=((16, 16, 32), (32, 32, 64)), num_centroids=(64, 16),
              radius=(0.2, 0.4), max_neighbors=(8, 8), fp_channels=((32, 32), (32, 16)), fp_neighbors=(3, 3),
              seg_channels=(16,), dropout_prob=0.0)


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def pn2():
    import mvkpconv
    return mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg"), mvkpconv.sub("dropin.mvpnet.models.pn2.modules")


def test_library_exports_the_fused_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in ("mvk_pn2_mlp_supported", "mvk_pn2_sa_fwd", "mvk_pn2_fp_fwd"):
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9


def sa_args(c=2, n=8, m=4, k=3, widths=(5, 6)):
    params = torch.zeros(sum(widths[i + 1] * (widths[i] + 1) for i in range(len(widths) - 1)))
    return [torch.zeros(1, 3, n), torch.zeros(1, c, n), torch.zeros(1, 3, m), torch.zeros(1, m, k, dtype=torch.int64), params,
            widths]


def fp_args(c2=2, c1=3, n2=5, n1=8, widths=(5, 6)):
    params = torch.zeros(sum(widths[i + 1] * (widths[i] + 1) for i in range(len(widths) - 1)))
    return [torch.zeros(1, c2, n2), torch.zeros(1, n1, 3, dtype=torch.int64), torch.zeros(1, n1, 3), torch.zeros(1, c1, n1),
            params, widths]


@pytest.mark.parametrize("which", ["sa", "fp"])
def test_wrappers_refuse_what_they_do_not_run(ops, which):
    fn, make = (ops.pn2_sa_mlp_max, sa_args) if which == "sa" else (ops.pn2_fp_mlp, fp_args)
    with pytest.raises(RuntimeError, match="HBM"):              # CPU tensors, like the other pn2 wrappers
        fn(*make())
    for pos in (0, 2, 4):                                       # a float64 operand, the packed parameters included
        a = make()
        a[pos] = a[pos].double()
        with pytest.raises(RuntimeError, match="float32"):
            fn(*a)
    a = make()
    a[3 if which == "fp" else 1] = torch.zeros(1, 8, 3).transpose(1, 2)         # (1,3,8) values, not contiguous
    with pytest.raises(RuntimeError, match="contiguous"):
        fn(*a)
    a = make()
    a[1] = a[1].int() if which == "fp" else a[1]
    a[3] = a[3].int() if which == "sa" else a[3]
    with pytest.raises(RuntimeError, match="int64"):
        fn(*a)
    a = make()
    a[4].requires_grad_(True)
    with pytest.raises(RuntimeError, match="no backward"):
        fn(*a)
    with torch.no_grad():                                       # with gradients off the same call gets as far as the device check
        with pytest.raises(RuntimeError, match="HBM"):
            fn(*a)


def test_supported_widths_cover_the_default_network_and_stop_at_the_lds(ops):
    default = [(67, 32, 32, 64), (67, 64, 64, 128), (131, 128, 128, 256), (259, 256, 256, 512), (768, 256, 256),
               (384, 256, 256), (320, 256, 128), (128, 128, 128, 128), (128, 128, 20), (3, 7), (9, 33)]
    assert all(ops.pn2_mlp_supported(w) for w in default)
    assert not ops.pn2_mlp_supported((8, 8, 8, 8, 8))           # four layers
    assert not ops.pn2_mlp_supported((769, 8)) and not ops.pn2_mlp_supported((8, 513))
    assert not ops.pn2_mlp_supported((768, 512, 512))           # 32 rows of 768 + 512 values do not fit 160 KiB
    assert not ops.pn2_mlp_supported((8,)) and not ops.pn2_mlp_supported((8, 0))


def perturbed_net(pn2, golden, **kw):
    """The g16 PointNet++ (its fixture weights have BatchNorm away from the initial values) on the CPU."""
    net = pn2[0].PN2SSG(**dict(NET_KW, **kw))
    if not kw:
        g16 = golden("g16_pn2ssg")
        net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g16.items() if k.startswith("sd/")}, strict=True)
    return net.eval()


def test_folded_parameters_equal_a_float64_numpy_fold(pn2, golden):
    net = perturbed_net(pn2, golden)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    assert np.abs(sd["sa_modules.0.mlp.0.bn.running_mean"]).max() > 0.01        # the statistics are not the initial ones
    keys = list(net.state_dict().keys())
    assert pn2[1].freeze_inference(net) is net and pn2[0].freeze_inference is pn2[1].freeze_inference
    assert list(net.state_dict().keys()) == keys
    stacks = [(net.sa_modules[i], "sa_modules.%d.mlp" % i, 3, None) for i in range(2)] + \
             [(net.fp_modules[i], "fp_modules.%d.mlp" % i, 2, None) for i in range(2)] + [(net, "mlp_seg", 1, "seg_logit")]
    for module, prefix, n, head in stacks:
        params, widths = module._frozen
        want, want_widths = ref.fold_stack(sd, prefix, n, head)
        assert tuple(widths) == want_widths and params.dtype == torch.float32 and params.is_contiguous()
        got = params.numpy()
        assert got.shape == want.shape
        # float64 on both sides, rounded to float32 once: at most one float32 spacing apart (torch and NumPy may round
        # the square root and the division of the float64 fold differently in the last float64 bit)
        assert np.all(np.abs(got.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)), prefix
    assert net.sa_modules[0]._frozen[1] == (7, 16, 16, 32) and net._frozen[1] == (16, 16, 5)
    # train() drops the snapshot of the module it is called on; eval() keeps the others
    net.sa_modules[1].train()
    assert net.sa_modules[1]._frozen is None and net.sa_modules[0]._frozen is not None
    net.eval()
    assert net.sa_modules[0]._frozen is not None
    net.train()
    assert all(m._frozen is None for m in net.modules() if isinstance(m, pn2[1].Freezable))
    pn2[1].freeze_inference(net.eval())
    assert pn2[1].unfreeze_inference(net) is net and net._frozen is None and net.fp_modules[0]._frozen is None


def test_modules_the_kernels_do_not_cover_are_left_alone(pn2, golden):
    net = perturbed_net(pn2, golden, num_centroids=(64, 0), fp_neighbors=(0, 3))
    pn2[1].freeze_inference(net)
    assert net.sa_modules[0]._frozen is not None and net.sa_modules[1]._frozen is None      # one group of every point
    assert net.fp_modules[0]._frozen is None and net.fp_modules[1]._frozen is not None      # broadcast, no 3-NN
    deep = perturbed_net(pn2, golden, sa_channels=((8, 8, 8, 8), (8, 8)), seg_channels=(8, 8, 8))
    pn2[1].freeze_inference(deep)
    assert deep.sa_modules[0]._frozen is None and deep.sa_modules[1]._frozen is not None     # four layers
    assert deep._frozen is None                                                              # three layers + the logits
    wide = perturbed_net(pn2, golden, sa_channels=((8, 600), (8, 8)))
    pn2[1].freeze_inference(wide)
    assert wide.sa_modules[0]._frozen is None and wide.sa_modules[1]._frozen is not None     # a layer wider than 512


def test_restatement_agrees_with_a_plain_torch_shared_mlp_and_max():
    import mvkpconv
    cnn = mvkpconv.sub("dropin.common.nn")
    rng = np.random.default_rng(5)
    b, c, n, m, k = 2, 3, 9, 4, 5
    mlp = cnn.SharedMLP(c + 3, (6, 7), ndim=2, bn=True).double().eval()
    with torch.no_grad():
        for layer in mlp:
            layer.bn.weight.copy_(torch.from_numpy(1 + 0.1 * rng.standard_normal(layer.bn.weight.shape)))
            layer.bn.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(layer.bn.bias.shape)))
            layer.bn.running_mean.copy_(torch.from_numpy(0.1 * rng.standard_normal(layer.bn.bias.shape)))
            layer.bn.running_var.copy_(torch.from_numpy(1 + 0.1 * np.abs(rng.standard_normal(layer.bn.bias.shape))))
    xyz, feature = rng.random((b, 3, n)), rng.standard_normal((b, c, n))
    new_xyz = rng.random((b, 3, m))
    index = rng.integers(0, n, size=(b, m, k))
    index[0, 1, 2:] = -1                                        # a tail and a whole row without a neighbour
    index[1, 3] = -1
    sd = {"mlp." + key: v.numpy() for key, v in mlp.state_dict().items()}
    params, widths = ref.fold_stack(sd, "mlp", 2, dtype=np.float64)
    got = ref.sa_mlp_max(xyz, feature, new_xyz, index, params, widths)

    def grouped(points):                                        # (b,C,n) -> (b,C,m,k), zero where the index is -1
        t, idx = torch.from_numpy(points), torch.from_numpy(index)
        flat = idx.clamp(min=0).reshape(b, 1, m * k).expand(-1, t.shape[1], -1)
        return torch.gather(t, 2, flat).reshape(b, -1, m, k) * (idx >= 0).unsqueeze(1)

    with torch.no_grad():
        x = torch.cat([grouped(feature), grouped(xyz) - torch.from_numpy(new_xyz).unsqueeze(-1)], dim=1)
        want = torch.max(mlp(x), dim=3)[0].numpy()
    assert got.shape == want.shape == (b, 7, m)
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13)
    # the propagation form with index None is the same chain on plain rows
    dense = rng.standard_normal((b, c + 3, n))
    mlp1 = cnn.SharedMLP(c + 3, (6, 7), ndim=1, bn=True).double().eval()
    mlp1.load_state_dict({key: (v.squeeze(-1) if v.dim() == 4 else v) for key, v in mlp.state_dict().items()})
    with torch.no_grad():
        want1 = mlp1(torch.from_numpy(dense)).numpy()
    np.testing.assert_allclose(ref.fp_mlp(None, None, None, dense, params, widths), want1, rtol=1e-12, atol=1e-13)
