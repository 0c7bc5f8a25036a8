"""CPU-only: the host side of the fused PointNet++ training path (csrc/pn2_rows.hip, ops.pn2_sa_rows / pn2_rows_max,
fuse_training): exports at ABI 9, the wrappers' refusals, the plain-attribute switch, and the NumPy restatement of
tests/pn2_train_ref.py against torch float64 gather + cat + max and its autograd."""
import ctypes

import numpy as np
import pytest
import torch

import pn2_train_ref as ref
from pn2_ordered_ref import ball_like_index, ordered_sum_loop

TRAIN_EXPORTS = ("mvk_pn2_sa_rows_fwd", "mvk_pn2_sa_rows_bwd", "mvk_pn2_sa_rows_bwd_csr", "mvk_pn2_rows_max_fwd",
                 "mvk_pn2_rows_max_bwd")
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


def test_library_exports_the_training_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in TRAIN_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header, name
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    # the row limit is a host check: refused with the library's argument error before any launch
    lib = lib_mod.lib()
    word = ctypes.c_int32(0)
    p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    assert lib.mvk_pn2_sa_rows_fwd(p, p, p, p, 2, 4, 1, 8, 1 << 25, 32, p, None) == -1
    assert "2^31" in lib.mvk_last_error().decode()
    assert lib.mvk_pn2_sa_rows_bwd(p, p, 2, 4, 8, 1 << 25, 32, p, None) == -1
    assert lib.mvk_pn2_sa_rows_bwd_csr(p, p, p, 2, 4, 8, 1 << 25, 32, p, None) == -1
    assert lib.mvk_pn2_rows_max_fwd(p, 2, 1 << 25, 32, 4, p, p, None) == -1
    assert "2^31" in lib.mvk_last_error().decode()
    assert lib.mvk_pn2_rows_max_bwd(p, p, 2, 1 << 25, 32, 4, p, None) == -1
    assert lib.mvk_pn2_rows_max_fwd(p, 2, 8, 0, 4, p, p, None) == -1            # K >= 1
    # empty problems launch nothing
    assert lib.mvk_pn2_sa_rows_fwd(None, None, None, None, 0, 4, 1, 8, 8, 4, None, None) == 0
    assert lib.mvk_pn2_rows_max_fwd(None, 0, 8, 4, 4, None, None, None) == 0


@pytest.mark.parametrize("which", ["rows", "max"])
def test_wrappers_refuse_what_they_do_not_run(ops, which):
    xyz, feat, new = torch.zeros(2, 3, 9), torch.zeros(2, 4, 9), torch.zeros(2, 3, 5)
    index = torch.zeros(2, 5, 3, dtype=torch.int64)
    y = torch.zeros(2 * 5 * 3, 6)
    if which == "rows":
        with pytest.raises(RuntimeError, match="HBM"):
            ops.pn2_sa_rows(xyz, feat, new, index)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_sa_rows(xyz, feat.double(), new, index)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_sa_rows(xyz.half(), None, new, index)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_sa_rows(xyz, torch.zeros(2, 9, 4).transpose(1, 2), new, index)
        with pytest.raises(RuntimeError, match="index must be int64"):
            ops.pn2_sa_rows(xyz, feat, new, index.int())
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_sa_rows(xyz, feat, new, torch.zeros(2, 3, 5, dtype=torch.int64).transpose(1, 2))
    else:
        with pytest.raises(RuntimeError, match="HBM"):
            ops.pn2_rows_max(y, 2, 5, 3)
        with pytest.raises(RuntimeError, match="must be float32"):
            ops.pn2_rows_max(y.double(), 2, 5, 3)
        with pytest.raises(RuntimeError, match="contiguous"):
            ops.pn2_rows_max(torch.zeros(6, 30).t(), 2, 5, 3)


def torch_group(points, index):
    """group_points on the host: (B,C,N), (B,M,K) -> (B,C,M,K), zero where the index is outside [0, N)."""
    b, c, n = points.shape
    ok = (index >= 0) & (index < n)
    j = index.clamp(0, n - 1).reshape(b, 1, -1).expand(-1, c, -1)
    return torch.gather(points, 2, j).reshape(b, c, *index.shape[1:]) * ok[:, None].to(points.dtype)


@pytest.mark.parametrize("with_feature, use_xyz", [(True, True), (True, False), (False, True)])
def test_restatement_agrees_with_torch_float64(with_feature, use_xyz):
    rng = np.random.default_rng(7)
    b, n, m, k, c, cout = 2, 20, 6, 5, 4, 7
    index = ball_like_index(b, m, k, n, seed=11)
    assert (index == -1).any() and (index[..., -1] == index[..., 0]).any()
    xyz, new_xyz = rng.standard_normal((b, 3, n)), rng.standard_normal((b, 3, m))
    feature = rng.standard_normal((b, c, n)) if with_feature else None
    cin = (c if with_feature else 0) + (3 if use_xyz or not with_feature else 0)
    w, go = rng.standard_normal((cout, cin)), rng.standard_normal((b, cout, m))
    # torch float64: QueryGrouper's tensors, a 1x1 convolution, the max over the neighbours, autograd
    ft = torch.from_numpy(feature).requires_grad_(True) if with_feature else None
    ix = torch.from_numpy(index)
    gx = torch_group(torch.from_numpy(xyz), ix) - torch.from_numpy(new_xyz).unsqueeze(-1)
    grouped = gx if ft is None else (torch.cat([torch_group(ft, ix), gx], 1) if use_xyz else torch_group(ft, ix))
    assert grouped.shape == (b, cin, m, k)
    conv = torch.einsum("oc,bcmk->bomk", torch.from_numpy(w), grouped)
    out_t = conv.max(dim=3)[0]
    # the restatement, in float64
    x = ref.sa_rows(xyz, feature, new_xyz, index, use_xyz)
    assert x.shape == (cin, b * m * k) and x.dtype == np.float64
    assert np.array_equal(x.reshape(cin, b, m, k), grouped.detach().numpy().transpose(1, 0, 2, 3))      # bit for bit
    y = x.T @ w.T
    out, arg = ref.rows_max(y, b, m, k)
    assert arg.dtype == np.int32 and out.shape == (b, cout, m)
    np.testing.assert_allclose(out, out_t.detach().numpy(), rtol=1e-13, atol=1e-13)
    t = y.reshape(b, m, k, cout)
    assert np.array_equal(out, t.max(axis=2).transpose(0, 2, 1))
    first = (t == t.max(axis=2, keepdims=True)).argmax(axis=2).transpose(0, 2, 1)
    assert np.array_equal(arg, first) and (t[:, :, 0] == t[:, :, -1]).any()    # padded rows: equal maxima do occur
    if with_feature:
        (out_t * torch.from_numpy(go)).sum().backward()
        dy = ref.rows_max_bwd(go, arg, k)
        assert np.count_nonzero(dy) == go.size and not np.signbit(dy[dy == 0]).any()
        df = ref.sa_rows_bwd(np.ascontiguousarray((dy @ w).T), index, c, n)
        np.testing.assert_allclose(df, ft.grad.numpy(), rtol=1e-12, atol=1e-12)
        wide, scale, count = ref.sa_rows_bwd_wide(np.ascontiguousarray((dy @ w).T), index, c, n)
        assert np.array_equal(wide, df) and np.all(scale >= np.abs(wide) - 1e-12)
        assert count.sum() == int(((index >= 0) & (index < n)).sum())


def test_ordered_rows_backward_is_the_sequential_float32_sum():
    rng = np.random.default_rng(5)
    b, n, m, k, c = 2, 11, 40, 5, 3
    index = ball_like_index(b, m, k, n, seed=4)
    dx = rng.standard_normal((c + 3, b * m * k)).astype(np.float32)
    got = ref.sa_rows_bwd(dx, index, c, n)
    assert got.dtype == np.float32 and got.shape == (b, c, n)
    for bi, ci in ((0, 0), (1, 2)):
        want = ordered_sum_loop(dx[ci].reshape(b, -1)[bi], index[bi].reshape(-1), n)
        assert np.array_equal(got[bi, ci].view(np.int32), want.view(np.int32))
    # a NaN propagates through the max and is found at its first row
    y = rng.standard_normal((1 * 2 * 4, 3)).astype(np.float32)
    y[5, 1] = y[6, 1] = np.nan
    out, arg = ref.rows_max(y, 1, 2, 4)
    assert np.isnan(out[0, 1, 1]) and arg[0, 1, 1] == 1 and not np.isnan(out[0, :, 0]).any()


def cpu_ball_query(new_xyz, xyz, radius, k, key_lengths=None):
    d2 = ((new_xyz.unsqueeze(3) - xyz.unsqueeze(2)) ** 2).sum(1)             # (B,M,N)
    index = torch.full(d2.shape[:2] + (k,), -1, dtype=torch.int64)
    for b in range(d2.shape[0]):
        for m in range(d2.shape[1]):
            hits = torch.nonzero(d2[b, m] < radius * radius)[:k, 0]
            if len(hits):
                index[b, m] = hits[0]
                index[b, m, :len(hits)] = hits
    return index


def test_fuse_training_is_a_plain_attribute_and_leaves_eval_mode_alone(ops, pn2, monkeypatch):
    pn2ssg, modules = pn2
    assert pn2ssg.fuse_training is modules.fuse_training and pn2ssg.unfuse_training is modules.unfuse_training
    torch.manual_seed(1)
    net = pn2ssg.PN2SSG(**NET_KW)
    keys = list(net.state_dict().keys())
    fusable = [m for m in net.modules() if isinstance(m, modules.FusableTraining)]
    assert len(fusable) == 5 and not any(m._fused_training for m in fusable)
    assert modules.fuse_training(net) is net and all(m._fused_training for m in fusable)
    assert list(net.state_dict().keys()) == keys
    assert all(modules.rows_stack(m.mlp) for m in fusable[1:]) and modules.rows_stack(net.mlp_seg)
    assert not modules.rows_stack(type(net.mlp_seg)(8, (8,), ndim=1, bn=False))           # a stack without BatchNorm
    # a CPU tensor, float64, eval mode: the PyTorch layers
    sa = net.sa_modules[0]
    assert not sa._use_fused_training(sa.mlp, torch.zeros(1, 3, 4))
    net.eval()
    assert not any(m._use_fused_training(m.mlp if hasattr(m, "mlp") else m.mlp_seg) for m in fusable)
    # eval mode with both switches on: the frozen path under no_grad, the PyTorch layers with gradients; never the rows
    modules.freeze_inference(net)
    assert sa._frozen is not None and sa._fused_training
    calls = {"frozen": 0, "rows": 0}

    def frozen_stand_in(xyz, feature, new_xyz, index, params, widths):
        calls["frozen"] += 1
        return torch.zeros(xyz.shape[0], widths[-1], new_xyz.shape[2])

    def rows_stand_in(*a, **k):
        calls["rows"] += 1
        raise AssertionError("the fused training path ran in eval mode")

    monkeypatch.setattr(ops, "pn2_sa_mlp_max", frozen_stand_in)
    monkeypatch.setattr(ops, "pn2_sa_rows", rows_stand_in)
    monkeypatch.setattr(modules, "farthest_point_sample",
                        lambda xyz, n, lengths=None: torch.arange(n).repeat(xyz.shape[0], 1))
    monkeypatch.setattr(modules, "ball_query", cpu_ball_query)
    monkeypatch.setattr(modules, "group_points", torch_group)
    rng = np.random.default_rng(2)
    xyz = torch.from_numpy(rng.random((2, 3, 80)).astype(np.float32))
    feat = torch.from_numpy(rng.standard_normal((2, 4, 80)).astype(np.float32))
    with torch.no_grad():
        _, out = sa(xyz, feat)
    assert calls == {"frozen": 1, "rows": 0} and out.shape == (2, 32, 64)
    _, out = sa(xyz, feat)                                                     # gradients on: not frozen, not fused
    assert calls == {"frozen": 1, "rows": 0} and out.shape == (2, 32, 64) and out.requires_grad
    net.train()
    assert sa._frozen is None and sa._fused_training                           # train() drops the snapshot only
    assert modules.unfuse_training(net) is net and not any(m._fused_training for m in fusable)
    assert list(net.state_dict().keys()) == keys
