"""CPU-only: the host side of the fused FeatureAggregation training path (csrc/pn2_rows.hip, ops.pn2_fa_rows /
pn2_rows_sum, fuse_training(net, aggregation=True)): exports at ABI 9, the size refusals through the raw library, the
wrappers' refusals, the plain-attribute switch, and the NumPy restatement of tests/fa_train_ref.py against the unfused
function written in torch float64 (gather + subtraction + cat + a 1x1 product + sum / max) and its autograd."""
import ctypes

import numpy as np
import pytest
import torch

import fa_train_ref as ref
from pn2_train_ref import rows_max, rows_max_bwd
from test_pn2_train_cpu import torch_group

FA_EXPORTS = ("mvk_pn2_fa_rows_fwd", "mvk_pn2_fa_rows_bwd", "mvk_pn2_fa_rows_bwd_csr", "mvk_pn2_rows_sum_fwd",
              "mvk_pn2_rows_sum_bwd")


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def dropin():
    import mvkpconv
    return mvkpconv.sub


def test_library_exports_the_aggregation_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in FA_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header, name
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    lib = lib_mod.lib()
    word = ctypes.c_int32(0)
    p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    # R = B*np*k = 2 * 2^25 * 32 = 2^31 rows: a host check, refused with the library's argument error before any launch
    assert lib.mvk_pn2_fa_rows_fwd(p, 64, 8, 1, p, p, p, 2, 1, 4, 8, 1 << 25, 32, 1, p, None) == -1
    assert "2^31" in lib.mvk_last_error().decode() and "B*np*k" in lib.mvk_last_error().decode()
    assert lib.mvk_pn2_fa_rows_bwd(p, p, 2, 1, 4, 8, 1 << 25, 32, p, 64, 8, 1, None) == -1
    assert lib.mvk_pn2_fa_rows_bwd_csr(p, p, p, 2, 1, 4, 8, 1 << 25, 32, p, 64, 8, 1, None) == -1
    # B*nv*hw = 2 * 4 * 2^28 = 2^31 pixels
    assert lib.mvk_pn2_fa_rows_fwd(p, 64, 8, 1, p, p, p, 2, 4, 4, 1 << 28, 8, 3, 1, p, None) == -1
    assert "2^31" in lib.mvk_last_error().decode() and "B*nv*hw" in lib.mvk_last_error().decode()
    assert lib.mvk_pn2_fa_rows_bwd(p, p, 2, 4, 4, 1 << 28, 8, 3, p, 64, 8, 1, None) == -1
    assert lib.mvk_pn2_fa_rows_bwd_csr(p, p, p, 2, 4, 4, 1 << 28, 8, 3, p, 64, 8, 1, None) == -1
    assert lib.mvk_pn2_rows_sum_fwd(p, 2, 1 << 25, 32, 4, p, None) == -1
    assert "2^31" in lib.mvk_last_error().decode()
    assert lib.mvk_pn2_rows_sum_bwd(p, 2, 1 << 25, 32, 4, p, None) == -1
    assert lib.mvk_pn2_rows_sum_fwd(p, 2, 8, 0, 4, p, None) == -1                  # K >= 1
    # empty problems launch nothing
    assert lib.mvk_pn2_fa_rows_fwd(None, 0, 0, 0, None, None, None, 0, 2, 4, 8, 8, 3, 1, None, None) == 0
    assert lib.mvk_pn2_fa_rows_fwd(None, 0, 0, 0, None, None, None, 2, 2, 4, 8, 0, 3, 1, None, None) == 0
    assert lib.mvk_pn2_fa_rows_bwd(None, None, 2, 2, 4, 8, 8, 0, None, 0, 0, 0, None) == 0
    assert lib.mvk_pn2_fa_rows_bwd_csr(None, None, None, 2, 2, 0, 8, 8, 3, None, 0, 0, 0, None) == 0
    assert lib.mvk_pn2_rows_sum_fwd(None, 0, 8, 4, 4, None, None) == 0
    assert lib.mvk_pn2_rows_sum_bwd(None, 2, 0, 4, 4, None, None) == 0


@pytest.mark.parametrize("which", ["rows", "sum"])
def test_wrappers_refuse_what_they_do_not_run(ops, which):
    fmap, xyz, pts = torch.zeros(4, 5, 2, 3), torch.zeros(2, 2, 2, 3, 3), torch.zeros(2, 3, 7)
    index = torch.zeros(2, 7, 3, dtype=torch.int64)
    y = torch.zeros(2 * 7 * 3, 6)
    if which == "rows":
        with pytest.raises(RuntimeError, match="HBM"):
            ops.pn2_fa_rows(fmap, xyz, pts, index)
        with pytest.raises(RuntimeError, match="HBM"):
            ops.pn2_fa_rows(fmap.contiguous(memory_format=torch.channels_last), xyz, pts, index)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_fa_rows(fmap.double(), xyz, pts, index)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_fa_rows(fmap, xyz.half(), pts, index)
        with pytest.raises(RuntimeError, match=r"expected feature_2d \(B\*nv,C,h,w\)"):
            ops.pn2_fa_rows(fmap[0], xyz, pts, index)
        with pytest.raises(RuntimeError, match="contiguous or channels-last"):
            ops.pn2_fa_rows(torch.zeros(4, 5, 3, 2).transpose(2, 3), xyz, pts, index)      # strides (30, 6, 1, 2)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_fa_rows(fmap, xyz, torch.zeros(2, 7, 3).transpose(1, 2), index)
        with pytest.raises(RuntimeError, match="index must be int64"):
            ops.pn2_fa_rows(fmap, xyz, pts, index.int())
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_fa_rows(fmap, xyz, pts, torch.zeros(2, 3, 7, dtype=torch.int64).transpose(1, 2))
    else:
        with pytest.raises(RuntimeError, match="HBM"):
            ops.pn2_rows_sum(y, 2, 7, 3)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_rows_sum(y.double(), 2, 7, 3)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_rows_sum(torch.zeros(6, 42).t(), 2, 7, 3)


def dyadic(rng, shape):
    return (rng.integers(0, 64, size=shape) / 64.0).astype(np.float32)


@pytest.mark.parametrize("reduction, use_relation", [("sum", True), ("max", True), ("sum", False)])
def test_restatement_agrees_with_torch_float64(reduction, use_relation):
    rng = np.random.default_rng(17)
    b, nv, h, w, c, n, k, cout = 2, 2, 3, 4, 5, 9, 3, 7
    p_all = nv * h * w
    index = rng.integers(0, p_all, size=(b, n, k)).astype(np.int64)
    index[0, 0] = -1                                             # a row of -1
    index[1, 2, 1] = p_all                                       # one index past the end
    index[1, 3:, :2] = 5                                         # one pixel hit by many points
    assert (index < 0).any() and (index >= p_all).any() and (index[1] == 5).sum() >= 2 * (n - 3)
    fmap, image_xyz, points = dyadic(rng, (b * nv, c, h, w)), dyadic(rng, (b, nv, h, w, 3)), dyadic(rng, (b, 3, n))
    cin = c + (4 if use_relation else 0)
    wgt, go = rng.standard_normal((cout, cin)), rng.standard_normal((b, cout, n))
    # torch float64: MVPNet3D.forward's transposed copy and two group_points, FeatureAggregation.forward's tensors, a 1x1
    # convolution, the reduction over k, autograd
    ft = torch.from_numpy(fmap.astype(np.float64)).requires_grad_(True)
    ix = torch.from_numpy(index)
    planes = ft.reshape(b, nv, c, h, w).transpose(1, 2).reshape(b, c, p_all)
    grouped = torch_group(planes, ix)
    if use_relation:
        xyz = torch.from_numpy(image_xyz.astype(np.float64)).permute(0, 4, 1, 2, 3).reshape(b, 3, p_all)
        diff = torch_group(xyz, ix) - torch.from_numpy(points.astype(np.float64)).unsqueeze(-1)
        grouped = torch.cat([grouped, diff, torch.sum(diff ** 2, dim=1, keepdim=True)], dim=1)
    assert grouped.shape == (b, cin, n, k)
    conv = torch.einsum("oc,bcmk->bomk", torch.from_numpy(wgt), grouped)
    out_t = conv.sum(dim=3) if reduction == "sum" else conv.max(dim=3)[0]
    # the restatement in float32 on the float32 inputs: dyadic values, so every difference, square and sum is exact and
    # the float32 rows are the float64 rows bit for bit
    x32 = ref.fa_rows(fmap, image_xyz, points, index, use_relation)
    assert x32.dtype == np.float32 and x32.shape == (cin, b * n * k)
    assert np.array_equal(x32.astype(np.float64).reshape(cin, b, n, k), grouped.detach().numpy().transpose(1, 0, 2, 3))
    assert not x32[:c, :k].any() and (not use_relation or np.array_equal(x32[c:c + 3, 0], -points[0, :, 0]))
    # ... and in float64, through the product, the reduction and both backwards
    x = ref.fa_rows(fmap.astype(np.float64), image_xyz.astype(np.float64), points.astype(np.float64), index, use_relation)
    assert x.dtype == np.float64 and np.array_equal(x, x32.astype(np.float64))
    y = x.T @ wgt.T
    if reduction == "sum":
        out = ref.rows_sum(y, b, n, k)
        dy = ref.rows_sum_bwd(go, k)
        assert np.array_equal(dy.reshape(b, n, k, cout)[:, :, k - 1], go.transpose(0, 2, 1))
    else:
        out, arg = rows_max(y, b, n, k)
        dy = rows_max_bwd(go, arg, k)
    np.testing.assert_allclose(out, out_t.detach().numpy(), rtol=1e-13, atol=1e-13)
    (out_t * torch.from_numpy(go)).sum().backward()
    dmap = ref.fa_rows_bwd(np.ascontiguousarray((dy @ wgt).T), index, c, nv, h, w)
    assert dmap.shape == fmap.shape
    np.testing.assert_allclose(dmap, ft.grad.numpy(), rtol=1e-12, atol=1e-12)
    wide, scale, count = ref.fa_rows_bwd_wide(np.ascontiguousarray((dy @ wgt).T), index, c, nv, h, w)
    assert np.array_equal(wide, dmap) and np.all(scale >= np.abs(wide) - 1e-12)
    assert count.shape == (b * nv, 1, h, w) and count.sum() == int(((index >= 0) & (index < p_all)).sum())
    assert count[1 * nv + 0, 0, 5 // w, 5 % w] >= 2 * (n - 3)


def test_ordered_backward_and_sum_are_sequential_float32_sums():
    from pn2_ordered_ref import ordered_sum_loop
    rng = np.random.default_rng(6)
    b, nv, h, w, c, n, k = 2, 2, 2, 3, 3, 40, 3
    p_all = nv * h * w
    index = rng.integers(-1, p_all + 1, size=(b, n, k)).astype(np.int64)
    dx = rng.standard_normal((c + 4, b * n * k)).astype(np.float32)
    got = ref.fa_rows_bwd(dx, index, c, nv, h, w)
    assert got.dtype == np.float32 and got.shape == (b * nv, c, h, w)
    for bi, ci in ((0, 0), (1, 2)):
        want = ordered_sum_loop(dx[ci].reshape(b, -1)[bi], index[bi].reshape(-1), p_all)
        assert np.array_equal(got[bi * nv:(bi + 1) * nv, ci].reshape(-1).view(np.int32), want.view(np.int32))
    y = rng.standard_normal((2 * 3 * 5, 4)).astype(np.float32)
    y[0:5, 0] = -0.0                                             # a point whose rows are all -0: the sum is -0
    y[7, 1] = np.nan
    out = ref.rows_sum(y, 2, 3, 5)
    assert out.dtype == np.float32 and np.signbit(out[0, 0, 0]) and out[0, 0, 0] == 0 and np.isnan(out[0, 1, 1])
    acc = y[10, 2]
    for j in range(11, 15):
        acc = np.float32(acc + y[j, 2])
    assert out[0, 2, 2] == acc


class MapEncoder(torch.nn.Module):
    """Stands for the 2D encoder: returns a stored map whatever the images are."""

    def __init__(self, fmap):
        super().__init__()
        self.map = torch.nn.Parameter(fmap)

    def forward(self, data):
        return {"feature": self.map}


def test_fuse_training_switches_the_aggregation_only_on_request(dropin):
    m3 = dropin("dropin.mvpnet.models.mvpnet_3d")
    pn2ssg = dropin("dropin.mvpnet.models.pn2.pn2ssg")
    modules = dropin("dropin.mvpnet.models.pn2.modules")
    torch.manual_seed(2)
    net_3d = pn2ssg.PN2SSG(8, 5, sa_channels=((16, 16),), num_centroids=(32,), radius=(0.3,), max_neighbors=(8,),
                           fp_channels=((16,),), fp_neighbors=(3,), seg_channels=(16,), dropout_prob=0.0)
    net = m3.MVPNet3D(MapEncoder(torch.zeros(6, 8, 6, 8)), None, net_3d, in_channels=8, mlp_channels=(8, 8))
    fa = net.feat_aggreg
    keys = list(net.state_dict().keys())
    assert isinstance(fa, modules.FusableTraining) and isinstance(fa, modules.Freezable) and not fa._fused_training
    assert pn2ssg.fuse_training(net) is net                     # the one-argument call: the 3D network only
    assert not fa._fused_training and net_3d._fused_training and net_3d.sa_modules[0]._fused_training
    assert pn2ssg.fuse_training(net, aggregation=True) is net and fa._fused_training
    assert list(net.state_dict().keys()) == keys and "_fused_training" not in fa.__dict__.get("_buffers", {})
    assert modules.rows_stack(fa.mlp)
    # CPU tensors, float64 and eval mode never take the rows
    cpu = torch.zeros(6, 8, 6, 8), torch.zeros(3, 2, 6, 8, 3), torch.zeros(3, 3, 4)
    assert net.training and not fa._use_rows(*cpu)
    net.eval()
    assert fa._fused_training and not fa._use_rows(*cpu)
    net.train()
    assert fa._fused_training                                    # train() drops the frozen snapshot only
    # a module without an MLP, or with another reduction, has no rows to run
    bare = m3.FeatureAggregation(8, mlp_channels=())
    pn2ssg.fuse_training(bare, aggregation=True)
    assert bare._fused_training and not bare._use_rows(*cpu)
    with pytest.raises(RuntimeError, match="needs an MLP"):
        bare.forward_rows(cpu[0], cpu[1], torch.zeros(3, 4, 3, dtype=torch.int64), cpu[2])
    assert pn2ssg.unfuse_training(net) is net and not fa._fused_training and not net_3d._fused_training
    assert list(net.state_dict().keys()) == keys
