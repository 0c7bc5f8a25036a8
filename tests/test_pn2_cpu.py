"""CPU-only: the NumPy restatements of the MVPNet baseline's point ops (tests/pn2_ref.py) against the outputs of the
reference's own restatements (fixture g15, tests/golden/make_pn2_golden.py), the tie rule of farthest point sampling,
and the built library's / the drop-in's side of the feature (exports, ABI 9, CPU tensors refused, import resolution)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import pn2_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FPS, N_BQ, N_KNN, N_ITP = 4, 4, 4, 2

PN2_EXPORTS = ("mvk_fps_workspace", "mvk_fps", "mvk_fps_f64", "mvk_pn2_ball_query", "mvk_pn2_ball_query_f64",
               "mvk_knn_distance", "mvk_knn_distance_f64", "mvk_interpolate_fwd", "mvk_interpolate_fwd_f64",
               "mvk_interpolate_bwd", "mvk_interpolate_bwd_f64")


@pytest.fixture(scope="module")
def g15(golden):
    return golden("g15_pn2_ops")


def rows(a, transpose):
    return np.ascontiguousarray(a.transpose(0, 2, 1)) if transpose else a


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_fps_restatements_reproduce_the_reference_restatement(g15, tag):
    for i in range(N_FPS):
        pts = rows(g15["fps%d_%s_points" % (i, tag)], bool(g15["fps%d_transpose" % i]))
        want = g15["fps%d_%s_index" % (i, tag)]
        # random clouds: the largest distance is never shared, so the tie rule and np.argmax agree
        assert np.array_equal(pn2_ref.fps_batch(pts, want.shape[1], pn2_ref.fps_closed), want)
        assert np.array_equal(pn2_ref.fps_batch(pts, want.shape[1], pn2_ref.fps_literal), want)


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_ball_query_restatement_reproduces_the_reference_restatement(g15, tag):
    for i in range(N_BQ):
        r, k, tr = g15["bq%d_radius_k_transpose" % i]
        q, ky = rows(g15["bq%d_%s_query" % (i, tag)], bool(tr)), rows(g15["bq%d_%s_key" % (i, tag)], bool(tr))
        index, distance = pn2_ref.ball_query(q, ky, float(r), int(k))
        assert np.array_equal(index, g15["bq%d_%s_index" % (i, tag)])
        # the reference's restatement stores its distances in a float32 array whatever the input dtype
        assert np.array_equal(distance.astype(np.float32), g15["bq%d_%s_distance" % (i, tag)])


@pytest.mark.parametrize("tag", ["f32", "f64"])
def test_knn_restatement_reproduces_topk_on_the_distance_matrix(g15, tag):
    for i in range(N_KNN):
        tr = bool(g15["knn%d_transpose" % i])
        q, ky = rows(g15["knn%d_%s_query" % (i, tag)], tr), rows(g15["knn%d_%s_key" % (i, tag)], tr)
        index, distance = pn2_ref.knn3(q, ky)
        assert np.array_equal(index, g15["knn%d_%s_index" % (i, tag)])
        # the reference's own test compares these distances with atol=1e-6 (torch.sum may add the three squares in
        # another order than the kernel)
        np.testing.assert_allclose(distance, g15["knn%d_%s_distance" % (i, tag)], rtol=0, atol=1e-6)


def test_interpolation_restatement_reproduces_the_reference_restatement(g15):
    for i in range(N_ITP):
        f, idx, w, go = (g15["itp%d_%s" % (i, n)] for n in ("feature", "index", "weight", "grad_out"))
        out, _ = pn2_ref.interpolate_fwd(f, idx, w)
        np.testing.assert_allclose(out, g15["itp%d_out" % i], rtol=1e-13, atol=1e-14)
        gi, _, count = pn2_ref.interpolate_bwd(go, idx, w, f.shape[2])
        np.testing.assert_allclose(gi, g15["itp%d_grad_feature" % i], rtol=1e-12, atol=1e-13)
        assert count.sum() == idx.size


@pytest.mark.parametrize("n, m, seed", pn2_ref.LATTICE_CASES)
def test_fps_schedule_simulation_equals_the_closed_form_on_lattice_clouds(n, m, seed):
    for dt in (np.float32, np.float64):
        pts = pn2_ref.lattice_cloud(n, seed).astype(dt)
        lit = pn2_ref.fps_literal(pts, m)
        assert np.array_equal(lit, pn2_ref.fps_closed(pts, m))
        if n == 1100:       # 125 distinct lattice points at most: the sample runs out and repeats its last index
            assert lit[-1] == lit[-2] and len(set(lit.tolist())) < m
        if n == 16:         # every DISTINCT point is chosen before the repeats begin
            assert len(set(map(tuple, pts[lit].tolist()))) == len(set(map(tuple, pts.tolist())))


def test_fps_tie_rule_is_not_argmax():
    n, m, seed = pn2_ref.LATTICE_CASES[0]
    pts = pn2_ref.lattice_cloud(n, seed)
    assert not np.array_equal(pn2_ref.fps_closed(pts, m), pn2_ref.fps_argmax(pts, m))


def test_reference_block_size_and_tie_key():
    assert [pn2_ref.ref_block(n) for n in (1, 15, 16, 31, 32, 70, 511, 512, 1100, 20000)] == \
        [16, 16, 16, 16, 32, 64, 256, 512, 512, 512]
    # 70 points -> blocks of 64: thread 32 (bit-reversed 1) beats thread 1 (bit-reversed 32); point 64 shares thread 0
    key = pn2_ref.tie_key(np.array([0, 1, 32, 64]), 70)
    assert key[0] < key[3] < key[2] < key[1]


def test_library_exports_the_pn2_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in PN2_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    # clouds that fit in registers need no workspace; larger ones one running distance per point
    assert lib_mod.lib().mvk_fps_workspace(4, 8192, 0) == 0 and lib_mod.lib().mvk_fps_workspace(4, 8192, 1) == 0
    assert lib_mod.lib().mvk_fps_workspace(2, 20000, 0) == 2 * 20000 * 4
    assert lib_mod.lib().mvk_fps_workspace(2, 20000, 1) == 2 * 20000 * 8


def test_pn2_wrappers_refuse_cpu_tensors():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    pts = torch.zeros(1, 8, 3)
    idx = torch.zeros(1, 8, 3, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.fps(pts, 2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.pn2_ball_query(pts, pts, 0.1, 4)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.knn_distance(pts, pts, 3)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.feature_interpolate(torch.zeros(1, 2, 8), idx, torch.zeros(1, 8, 3))
    fps_mod = mvkpconv.sub("dropin.mvpnet.ops.fps")
    with pytest.raises(RuntimeError, match="HBM"):
        fps_mod.farthest_point_sample(pts.transpose(1, 2), 2)


def test_shared_mlp_dropout_and_batch_index_select():
    import torch
    import mvkpconv
    cnn = mvkpconv.sub("dropin.common.nn")
    mlp = cnn.SharedMLPDO(4, (8, 6), ndim=1, bn=True, p=0.25)
    assert mlp.p == 0.25 and mlp.dropout_fn is torch.nn.functional.dropout and mlp.extra_repr() == "p=0.25"
    assert cnn.SharedMLPDO(4, (8,), ndim=2, p=0.5).dropout_fn is torch.nn.functional.dropout2d
    assert list(mlp.state_dict()) == list(cnn.SharedMLP(4, (8, 6), ndim=1, bn=True).state_dict())
    mlp.eval()
    x = torch.randn(2, 4, 5)
    with torch.no_grad():
        assert torch.equal(mlp(x), cnn.SharedMLP.forward(mlp, x))        # dropout is the identity in eval mode
    inp = torch.arange(2 * 3 * 5, dtype=torch.float32).view(2, 3, 5)
    index = torch.tensor([[4, 0], [1, 1]])
    got = cnn.batch_index_select(inp, index, dim=2)
    assert got.shape == (2, 3, 2) and torch.equal(got[0], inp[0][:, [4, 0]]) and torch.equal(got[1], inp[1][:, [1, 1]])


_STUB = {
    "mvpnet/__init__.py": "",
    "mvpnet/ops/__init__.py": "",
    "mvpnet/ops/fps.py": "raise ImportError('the reference mvpnet.ops.fps must be shadowed by the drop-in')\n",
    "mvpnet/ops/ball_query.py": "raise ImportError('the reference mvpnet.ops.ball_query must be shadowed by the drop-in')\n",
    "mvpnet/ops/knn_distance.py": "raise ImportError('the reference mvpnet.ops.knn_distance must be shadowed by the drop-in')\n",
    "mvpnet/ops/interpolate.py": "raise ImportError('the reference mvpnet.ops.interpolate must be shadowed by the drop-in')\n",
    "mvpnet/models/__init__.py": "",
    "mvpnet/models/pn2/__init__.py": "",
    "mvpnet/models/pn2/modules.py": "raise ImportError('the reference pn2.modules must be shadowed by the drop-in')\n",
    "mvpnet/models/pn2/pn2ssg.py": "raise ImportError('the reference pn2.pn2ssg must be shadowed by the drop-in')\n",
    "mvpnet/models/pn2/KPConv.py": "MARK = 'stub pn2.KPConv'\n",
    "common/__init__.py": "",
    "common/nn/__init__.py": "raise ImportError('the reference common.nn must be shadowed by the drop-in')\n",
    "common/nn/init.py": "MARK = 'stub common.nn.init'\n",
    "common/nn/functional.py": "MARK = 'stub common.nn.functional'\n",
}


def test_reference_import_statements_resolve_to_the_drop_in(tmp_path):
    """With dropin/ first on sys.path and a stub reference tree (own text) behind it: the imports at the head of the
    reference's pn2/modules.py and the PN2SSG import resolve to drop-in files, while common.nn.init / .functional and
    the reference's other pn2 modules still come from the tree behind."""
    import mvkpconv
    for rel, text in _STUB.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    dropin = os.path.join(ROOT, mvkpconv.PKG_NAME, "dropin")
    prog = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.append(%r)\n"
        "from common.nn import SharedMLP\n"
        "from common.nn import SharedMLPDO, batch_index_select\n"
        "from mvpnet.ops.fps import farthest_point_sample\n"
        "from mvpnet.ops.group_points import group_points\n"
        "from mvpnet.ops.ball_query import ball_query, ball_query_distance\n"
        "from mvpnet.ops.knn_distance import knn_distance\n"
        "from mvpnet.ops.interpolate import feature_interpolate\n"
        "from mvpnet.models.pn2.pn2ssg import PN2SSG\n"
        "from mvpnet.models.pn2.modules import QueryGrouper, SetAbstraction, FeatureInterpolator, FeaturePropagation\n"
        "from mvpnet.models.mvpnet_3d import MVPNet3D, FeatureAggregation\n"
        "import common.nn.init as I, common.nn.functional as Fn, mvpnet.models.pn2.KPConv as K\n"
        "for f in (farthest_point_sample, group_points, ball_query, ball_query_distance, knn_distance, feature_interpolate,\n"
        "          PN2SSG, SetAbstraction, MVPNet3D, SharedMLPDO, batch_index_select):\n"
        "    assert 'dropin' in sys.modules[f.__module__].__file__, f\n"
        "assert I.MARK.startswith('stub') and Fn.MARK.startswith('stub') and K.MARK.startswith('stub')\n"
        "net = PN2SSG(4, 5, sa_channels=((8, 8),), num_centroids=(4,), radius=(0.2,), max_neighbors=(4,),\n"
        "             fp_channels=((8,),), fp_neighbors=(3,), seg_channels=(8,))\n"
        "keys = list(net.state_dict())\n"
        "assert 'sa_modules.0.mlp.0.conv.weight' in keys and 'fp_modules.0.mlp.0.bn.running_var' in keys\n"
        "assert 'mlp_seg.0.conv.weight' in keys and 'seg_logit.bias' in keys and net.mlp_seg.p == 0.5\n"
        "print('PN2 IMPORTS OK')\n") % (dropin, str(tmp_path))
    r = subprocess.run([sys.executable, "-c", prog], cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=300)
    assert r.returncode == 0 and "PN2 IMPORTS OK" in r.stdout, r.stderr[-3000:]
