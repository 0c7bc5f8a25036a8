"""CPU-only: the NumPy restatement of the reference's voting (tests/vote_ref.py) on hand-worked cases, and the built
library's side of the feature (exports, ABI 9, the wrappers' refusal of CPU tensors)."""
import ctypes

import numpy as np
import pytest

import vote_ref


def test_overlapping_point_is_voted_twice_in_batch_order():
    # one cloud of 4 points, two spheres of it in ONE batch that share point 2; probabilities chosen as exact binary
    # fractions so that the hand-worked float64 values below are the exact products and sums
    votes = [np.zeros((4, 2))]
    probs = np.array([[0.25, 0.75], [0.5, 0.5],        # sphere 0: points 0, 2
                      [1.0, 0.0], [0.125, 0.875]],     # sphere 1: points 2, 3
                     np.float32)
    written = vote_ref.vote_batch(votes, probs, [2, 2], [0, 2, 2, 3], [0, 0], smooth=0.5)
    assert [w[1].tolist() for w in written] == [[0, 2], [2, 3]]
    want = np.array([[0.125, 0.375],
                     [0.0, 0.0],
                     [0.5 * (0.5 * 0.5) + 0.5 * 1.0, 0.5 * (0.5 * 0.5) + 0.0],    # first sphere's vote, then the second's
                     [0.0625, 0.4375]])
    assert np.array_equal(votes[0], want)
    # the order matters: the other order gives another value for the shared point
    other = [np.zeros((4, 2))]
    vote_ref.vote_batch(other, probs[[2, 3, 0, 1]], [2, 2], [2, 3, 0, 2], [0, 0], smooth=0.5)
    assert other[0][2, 0] == 0.5 * (0.5 * 1.0) + 0.5 * 0.5 and other[0][2, 0] != votes[0][2, 0]


def test_one_minus_smooth_is_the_double_difference():
    votes = [np.zeros((1, 1))]
    vote_ref.vote_batch(votes, np.ones((1, 1), np.float32), [1], [0], [0], smooth=0.95)
    assert votes[0][0, 0] == 1 - 0.95 and votes[0][0, 0] != 0.05


def test_radius_mask_in_float32():
    votes = [np.zeros((3, 1))]
    pts = np.array([[0.3, 0.0, 0.0], [0.0, 0.5, 0.0], [0.2, 0.2, 0.2]], np.float32)
    written = vote_ref.vote_batch(votes, np.ones((3, 1), np.float32), [3], [0, 1, 2], [0], points=pts, r2_max=0.2)
    assert written[0][1].tolist() == [0, 2]            # 0.09 and 0.12 vote, 0.25 does not
    assert votes[0][1, 0] == 0.0


def test_unvisited_row_with_an_ignored_first_label():
    label_values, ignored = np.array([0, 1, 2, 3]), [0]
    assert vote_ref.column_map(label_values, ignored).tolist() == [-1, 0, 1, 2]
    probs = np.array([[0.0, 0.0, 0.0], [0.2, 0.5, 0.3]])
    assert vote_ref.predict(probs, label_values, ignored).tolist() == [0, 2]
    # an ignored label in the middle, an exact tie (first maximum), a reprojection
    label_values, ignored = np.array([1, 4, 7, 9]), [7]
    assert vote_ref.widen(np.array([[0.4, 0.4, 0.2]]), label_values, ignored).tolist() == [[0.4, 0.4, 0.0, 0.2]]
    probs = np.array([[0.4, 0.4, 0.2], [0.1, 0.2, 0.7], [0.0, 0.0, 0.0]])
    assert vote_ref.predict(probs, label_values, ignored).tolist() == [1, 9, 1]
    assert vote_ref.predict(probs, label_values, ignored, proj=[1, 1, 0, 2]).tolist() == [9, 9, 1, 1]


def test_confusion_with_a_label_table_and_iou():
    label_values = [1, 4, 7]
    C = vote_ref.confusion([1, 1, 4, 7, 5, 4], [1, 4, 4, 7, 1, 1], label_values)     # truth 5 is outside the table
    assert C.tolist() == [[1, 1, 0], [1, 1, 0], [0, 0, 1]]
    assert vote_ref.drop_ignored(C, label_values, [4]).tolist() == [[1, 0], [0, 1]]
    got = vote_ref.iou(C)
    assert np.allclose(got, [1 / 3, 1 / 3, 1.0], atol=1e-6)
    # a class absent from the truth takes the mean IoU of the present ones
    got = vote_ref.iou(np.array([[2, 0], [0, 0]]))
    assert np.allclose(got, [1.0, 1.0], atol=1e-5)


def test_restatement_iou_equals_the_drop_in_metric():
    import mvkpconv
    metrics = mvkpconv.sub("dropin.utils.metrics")
    rng = np.random.default_rng(3)
    C = rng.integers(0, 50, size=(6, 6))
    C[4] = 0
    assert np.allclose(vote_ref.iou(C), metrics.IoU_from_confusions(C), rtol=0, atol=1e-12)


def test_softmax_restatement_sums_to_one():
    x = np.random.default_rng(0).standard_normal((100, 19)) * 3
    p64, p32 = vote_ref.softmax(x, np.float64), vote_ref.softmax(x, np.float32)
    assert p32.dtype == np.float32 and np.allclose(p64.sum(1), 1.0, atol=1e-14) and np.abs(p32 - p64).max() < 1e-6


def test_library_exports_the_vote_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    for name in ("mvk_vote_update", "mvk_vote_predict", "mvk_affine_lrelu"):
        assert name in lib_mod.EXPORTS
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    for name in ("mvk_vote_update", "mvk_vote_predict", "mvk_affine_lrelu"):
        assert hasattr(raw, name)
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    assert "#define MVK_ABI_VERSION 9" in header and "int mvk_vote_update(" in header


def test_wrappers_refuse_cpu_tensors_and_recorded_gradients():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    x = torch.zeros(4, 8, requires_grad=True)
    with pytest.raises(RuntimeError, match="forward only"):
        ops.affine_lrelu(x, torch.ones(8), torch.zeros(8))
    with torch.no_grad(), pytest.raises(RuntimeError, match="HBM"):
        ops.affine_lrelu(x, torch.ones(8), torch.zeros(8))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.vote_predict(torch.zeros(4, 3, dtype=torch.float64), torch.arange(3, dtype=torch.int32),
                         torch.arange(3, dtype=torch.int32))


def test_freeze_snapshot_lifecycle_on_the_cpu():
    """The structural half of the frozen forward that needs no GPU: plain attributes, same state-dict keys, dropped by
    train(), not taken with gradients enabled or on CPU rows."""
    import torch
    import mvkpconv
    blocks = mvkpconv.sub("dropin.models.blocks")
    net = torch.nn.Sequential(blocks.UnaryBlock(8, 16, True, 0.1), blocks.UnaryBlock(16, 4, False, 0.1))
    with torch.no_grad():
        bn = net[0].batch_norm.batch_norm
        bn.running_mean.normal_()
        bn.running_var.uniform_(0.5, 2.0)
        bn.weight.normal_(1.0, 0.1)
        bn.bias.normal_()
    keys = list(net.state_dict().keys())
    net.eval()
    x = torch.randn(5, 8)
    with torch.no_grad():
        before = net(x)
    blocks.freeze_inference(net)
    assert list(net.state_dict().keys()) == keys
    scale, shift = net[0].batch_norm._frozen[:2]
    want = bn.weight / torch.sqrt(bn.running_var + bn.eps)
    assert torch.allclose(scale, want, rtol=1e-6) and torch.allclose(shift, bn.bias - bn.running_mean * want, rtol=1e-5, atol=1e-6)
    assert torch.allclose(net[0]._frozen, net[0].mlp.weight * want[:, None], rtol=1e-6)
    assert net[1].__dict__.get("_frozen") is None                  # no BatchNorm, nothing to freeze
    with torch.no_grad():
        assert torch.equal(net(x), before)                          # CPU rows: the path is not taken
    net.train()
    assert net[0].__dict__.get("_frozen") is None and net[0].batch_norm.__dict__.get("_frozen") is None
    blocks.freeze_inference(net)
    blocks.unfreeze_inference(net)
    assert net[0].__dict__.get("_frozen") is None
