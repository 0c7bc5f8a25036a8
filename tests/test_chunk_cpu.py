"""CPU-only: the NumPy restatement of the MVPNet whole-scene test (tests/chunk_ref.py) against the reference's own outputs
(fixture g17, tests/golden/make_chunk_golden.py), and the built library's side of the feature (exports, ABI 9, drop-in
module paths, the wrappers' refusal of CPU tensors)."""
import ctypes

import numpy as np
import pytest

import chunk_ref
import util

C = 20


@pytest.fixture(scope="module")
def g17(golden):
    return golden("g17_mvpnet_chunks")


def test_the_dyadic_scene_is_the_fixtures_and_has_the_edge_cases(g17):
    p = chunk_ref.dyadic_scene()
    assert util.bits_equal(p, g17["points"]) and len(p) % 64 != 0 and 3000 < len(p) < 5000
    assert len(chunk_ref.corners(p)) == 12
    t = chunk_ref.thresholds(p)
    assert list(t) == g17["thresholds"].tolist()
    counts = chunk_ref.inner_counts(p)
    assert t[0] in counts and t[1] not in counts                  # the threshold IS one corner's count: >= keeps it
    # points exactly on chunk edges: the inclusive comparisons decide their membership
    cs = np.asarray(chunk_ref.CHUNK_SIZE)
    on_edge = 0
    for c in chunk_ref.corners(p):
        on_edge += int(((p[:, :2] == c) | (p[:, :2] == c + cs)).any(axis=1).sum())
    assert on_edge > 200


@pytest.mark.parametrize("k", [0, 1, 2])
def test_restatement_equals_the_reference_on_the_dyadic_scene(g17, k):
    p, t = g17["points"], "t%d/" % k
    thresh = int(g17["thresholds"][k])
    indices, bboxes = chunk_ref.scene2chunks(p, thresh=thresh)
    assert len(indices) == int(g17[t + "n_chunks"]) == (7, 6, 8)[k]
    assert [len(i) for i in indices] == g17[t + "sizes"].tolist()
    assert all(i.dtype == np.int64 for i in indices)
    assert np.array_equal(np.concatenate(indices), g17[t + "indices"])
    assert util.bits_equal(np.asarray(bboxes, np.float64), g17[t + "bboxes"])
    tables = chunk_ref.table_logits(int(g17["logit_seed"]) + k, C, [len(i) for i in indices])
    sums, visits, mean, pred = chunk_ref.vote_scene(len(p), C, zip(tables, indices))
    assert np.array_equal(visits, g17[t + "visits"]) and np.array_equal(pred, g17[t + "pred"])
    assert int((visits == 0).sum()) == (18, 277, 14)[k] and (pred[visits == 0] == C).all()
    if k == 0:
        assert util.bits_equal(mean, g17[t + "mean"])
    m = chunk_ref.evaluator_update(np.zeros((C, C)), pred, g17["labels"], C)
    assert np.array_equal(m, g17[t + "confusion"])
    assert util.bits_equal(np.asarray(chunk_ref.class_iou(m), np.float64), g17[t + "class_iou"])
    assert chunk_ref.overall_acc(m) == float(g17[t + "overall_acc"])


def test_restatement_on_hand_worked_cases():
    # 1 m scene: ceil((1 - 1.5) / 0.5) + 1 = 0 corners; 1.5 m scene: exactly one; one point: none
    assert chunk_ref.corners(chunk_ref.small_scene(0, 50, 1.0)) == []
    p = chunk_ref.small_scene(1, 50, 1.5)
    ind, box = chunk_ref.scene2chunks(p, thresh=1)
    assert len(ind) == 1 and ind[0].tolist() == list(range(50)) and box[0][[0, 1, 3, 4]].tolist() == [-0.2, -0.2, 1.7, 1.7]
    assert chunk_ref.scene2chunks(chunk_ref.small_scene(2, 1, 1.0), thresh=1) == ([], [])
    # vote: a padded chunk's extra columns do not vote, the first maximum wins, an unvisited row predicts C
    a = np.array([[1.0, 2.0, 9.0], [1.0, 0.5, 9.0]], np.float32)          # [C=2, ld=3], two indices: column 2 is padding
    b = np.array([[0.5], [2.0]], np.float32)
    sums, visits, mean, pred = chunk_ref.vote_scene(4, 2, [(a, [2, 0]), (b, [0])])
    assert sums.tolist() == [[2.5, 2.5], [0, 0], [1, 1], [0, 0]] and visits.tolist() == [2, 0, 1, 0]
    assert mean[0].tolist() == [1.25, 1.25] and pred.tolist() == [0, 2, 0, 2]
    # score: -100, -1 and truths >= C are dropped, and so is the no-prediction label C
    m = chunk_ref.confusion([0, 1, 1, -100, -1, 2, 5, 1], [0, 1, 0, 1, 1, 2, 1, 2], 2)
    assert m.tolist() == [[1, 0], [1, 1]]
    assert chunk_ref.evaluator_update(np.ones((2, 2)), [0, 1], [-100, -1], 2).tolist() == [[1, 1], [1, 1]]


def test_evaluator_on_numpy_input_equals_the_reference(g17):
    import mvkpconv
    ev_mod = mvkpconv.sub("dropin.mvpnet.evaluate_3d")
    names = ["c%d" % i for i in range(C)]
    for k in range(3):
        t = "t%d/" % k
        ev = ev_mod.Evaluator(names)
        labels = g17["labels"].copy()
        ev.update(g17[t + "pred"], labels)
        assert (labels[g17["labels"] == -100] == C).all()              # the reference's in-place rewrite, NumPy path
        assert ev.confusion_matrix.dtype == np.float64 and np.array_equal(ev.confusion_matrix, g17[t + "confusion"])
        assert util.bits_equal(np.asarray(ev.class_iou, np.float64), g17[t + "class_iou"])
        assert ev.overall_acc == float(g17[t + "overall_acc"]) and ev.overall_iou == float(g17[t + "overall_iou"])
        assert len(ev.class_seg_acc) == C
        assert "c3" in ev.print_table()
    ev = ev_mod.Evaluator(names)
    ev.update(np.zeros(8, np.int64), np.full(8, -100, np.int64))
    assert np.array_equal(ev.confusion_matrix, g17["all_negative_confusion"]) and not ev.confusion_matrix.any()
    # a label table that is not 0..C-1 (the reference's EVAL_CLASS_IDS scorer)
    ev = ev_mod.Evaluator(["a", "b", "c"], labels=[4, 9, 2])
    ev.batch_update([np.array([4, 9, 2, 2, 7, 4])], [np.array([4, 4, 2, 9, 4, 5])])
    assert ev.confusion_matrix.tolist() == [[1, 1, 0], [0, 0, 1], [0, 0, 1]]


def test_evaluator_save_table(tmp_path):
    import mvkpconv
    ev = mvkpconv.sub("dropin.mvpnet.evaluate_3d").Evaluator(["a", "b"])
    ev.update(np.array([0, 1, 1]), np.array([0, 1, 0]))
    ev.save_table(str(tmp_path / "eval.tsv"))
    head, row = open(str(tmp_path / "eval.tsv")).read().split("\n")
    assert head.split("\t") == ["overall acc", "overall iou", "a", "b"] and row.split("\t")[0] == "0.66667"


def test_library_exports_the_chunk_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    names = ("mvk_box_count", "mvk_box_select_workspace", "mvk_box_select", "mvk_chunk_vote_add", "mvk_chunk_vote_finish",
             "mvk_chunk_confusion")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in names:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    raw.mvk_box_select_workspace.restype = ctypes.c_int64
    raw.mvk_box_select_workspace.argtypes = [ctypes.c_int64, ctypes.c_int]
    assert raw.mvk_box_select_workspace(70000, 12) >= 69 * 12 * 4


def test_drop_in_modules_import_under_the_reference_paths():
    import mvkpconv
    cu = mvkpconv.sub("dropin.mvpnet.utils.chunk_util")
    ev = mvkpconv.sub("dropin.mvpnet.evaluate_3d")
    tm = mvkpconv.sub("dropin.mvpnet.test_mvpnet_3d")
    import inspect
    assert list(inspect.signature(cu.scene2chunks_legacy).parameters) == ["points", "chunk_size", "stride", "thresh", "margin",
                                                                          "return_bbox"]
    assert inspect.signature(cu.scene2chunks_legacy).parameters["thresh"].default == 1000
    assert list(inspect.signature(ev.Evaluator.__init__).parameters) == ["self", "class_names", "labels"]
    for name in ("WholeSceneVoter", "predict_whole_scene", "chunk_rgbd_inputs"):
        assert callable(getattr(tm, name))
    assert inspect.signature(tm.predict_whole_scene).parameters["min_nb_pts"].default == 2048


def test_wrappers_refuse_cpu_tensors():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    pts = torch.zeros(8, 3)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.box_count(pts, np.zeros((1, 4)))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.box_select(pts, np.zeros((1, 4)), [0])
    sums, counts = torch.zeros(8, 4), torch.zeros(8, dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_vote_add(sums, counts, torch.zeros(4, 2), torch.zeros(2, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_vote_finish(sums, counts)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_confusion(torch.zeros(8, dtype=torch.int64), torch.zeros(8, dtype=torch.int64), 4)
