"""CPU-only: the library's side of the whole-scene inputs (include/mvkpconv_scene.h parsed and bound beside the 133
functions of ABI 9, size refusals and empty problems through raw ctypes, wrappers that refuse CPU tensors) and the NumPy
restatements of tests/scene_inputs_ref.py against the reference's own frame choices (fixture g11)."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import chunk_ref
import scene_inputs_ref as ref

SCENE_EXPORTS = ("mvk_overlap_pack", "mvk_chunk_select_frames", "mvk_chunk_unproject", "mvk_scene_inputs_workspace",
                 "mvk_chunk_knn_many", "mvk_chunk_batch_rows")


@pytest.fixture(scope="module")
def L():
    import mvkpconv
    return mvkpconv.sub("_lib")


def test_second_header_parses_and_leaves_abi_9_alone(L):
    import mvkpconv
    text = open(mvkpconv._ROOT + "/include/mvkpconv_scene.h").read()
    functions, structs, constants = L.parse_header(text)
    assert tuple(functions) == SCENE_EXPORTS == tuple(L.SCENE_FUNCTIONS) and structs == {}
    assert constants == L.SCENE_CONSTANTS == {"MVK_SCENE_MAX_BASE": 524288, "MVK_SCENE_MAX_FRAMES": 4096}
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#ifndef MVKPCONV_SCENE_H" in code and "MVK_ABI_VERSION" not in code and code.count('extern "C"') == 1
    assert "uint32_t" not in code and "uint64_t" not in code
    for name, (ret, params) in functions.items():
        assert params[-1] == ("void*", "stream") or name == "mvk_scene_inputs_workspace"
        assert ret == ("int64_t" if name == "mvk_scene_inputs_workspace" else "int")
    # the first header's tables are what they were
    assert len(L.FUNCTIONS) == len(L.EXPORTS) == 133 and len(L.STRUCTS) == 6 and len(L.CONSTANTS) == 9
    assert L.ABI_VERSION == 9 and not set(SCENE_EXPORTS) & set(L.EXPORTS)


def test_scene_functions_are_exported_and_bound(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    assert lib.mvk_abi_version() == 9
    for name in SCENE_EXPORTS:
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(L.SCENE_FUNCTIONS[name][1])
        assert fn.restype is (ctypes.c_int64 if name == "mvk_scene_inputs_workspace" else ctypes.c_int)


def last_error(raw):
    raw.mvk_last_error.restype = ctypes.c_char_p
    return raw.mvk_last_error().decode()


def test_size_refusals_and_empty_problems_through_raw_ctypes(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    i64, i32, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_void_p
    one = ctypes.c_void_p(64)                                 # a non-null address that must never be touched
    raw.mvk_overlap_pack.argtypes = [vp, i64, i64, vp, vp]
    assert raw.mvk_overlap_pack(None, 0, 7, None, None) == 0 and raw.mvk_overlap_pack(None, 7, 0, None, None) == 0
    assert raw.mvk_overlap_pack(one, 1 << 20, 1 << 11, one, None) == -1 and "2^31" in last_error(raw)
    assert raw.mvk_overlap_pack(one, 1 << 31, 1, one, None) == -1

    raw.mvk_chunk_select_frames.argtypes = [vp, i64, i64, vp, vp, i64, vp, vp, i32, i32, vp, vp]
    assert raw.mvk_chunk_select_frames(None, 10, 3, None, None, 0, None, None, 0, 3, None, None) == 0     # no chunk
    assert raw.mvk_chunk_select_frames(None, 10, 3, None, None, 0, None, None, 4, 0, None, None) == 0     # no round
    assert raw.mvk_chunk_select_frames(one, 524289, 3, one, one, 5, one, one, 1, 3, one, None) == -1
    assert "524288" in last_error(raw) and "no fallback" in last_error(raw)
    assert raw.mvk_chunk_select_frames(one, 10, 4097, one, one, 5, one, one, 1, 3, one, None) == -1
    assert "4096" in last_error(raw)
    assert raw.mvk_chunk_select_frames(one, 10, 0, one, one, 5, one, one, 1, 3, one, None) == -1
    assert "no frame" in last_error(raw)
    assert raw.mvk_chunk_select_frames(one, 10, 3, one, one, 1 << 31, one, one, 1, 3, one, None) == -1

    raw.mvk_chunk_unproject.argtypes = [vp, i32, i32, vp, vp, vp, i64, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    assert raw.mvk_chunk_unproject(None, 0, 3, None, None, None, 5, 12, 16, None, None, None, None, None, None, None, None) == 0
    assert raw.mvk_chunk_unproject(one, 4, 3, one, one, one, 5, 1 << 15, 1 << 15, one, one, one, one, one, one, one, None) == -1
    assert "2^31" in last_error(raw)
    assert raw.mvk_chunk_unproject(one, -1, 3, one, one, one, 5, 12, 16, one, one, one, one, one, one, one, None) == -1

    raw.mvk_scene_inputs_workspace.restype = i64
    raw.mvk_scene_inputs_workspace.argtypes = [vp, i32, i64, i32]
    raw.mvk_knn_workspace.restype = i64
    raw.mvk_knn_workspace.argtypes = [i64, i64, i32]
    lens = np.array([1500, 40, 0, 2200], np.int64)
    want = max(raw.mvk_knn_workspace(int(n), 576, 3) for n in lens)
    assert raw.mvk_scene_inputs_workspace(lens.ctypes.data_as(vp), 4, 576, 3) == want
    assert raw.mvk_scene_inputs_workspace(None, 0, 576, 3) > 0

    raw.mvk_chunk_knn_many.argtypes = [vp, i64, vp, i64, vp, vp, vp, vp, i32, vp, vp, i64, i32, vp, vp, vp, i64, vp]
    assert raw.mvk_chunk_knn_many(None, 0, None, 0, None, None, None, None, 0, None, None, 0, 3, None, None, None, 0, None) == 0
    q_off = np.array([0, 0, 0], np.int64)
    zero = np.zeros(2, np.int64)
    assert raw.mvk_chunk_knn_many(one, 9, one, 9, one, one, zero.ctypes.data_as(vp), q_off.ctypes.data_as(vp), 2, one, one,
                                  100, 3, one, one, one, 0, None) == 0                                  # chunks without points
    assert raw.mvk_chunk_knn_many(one, 9, one, 9, one, one, zero.ctypes.data_as(vp), q_off.ctypes.data_as(vp), 2, one, one,
                                  100, 9, one, one, one, 0, None) == -1 and "k=9" in last_error(raw)
    bad = np.array([0, 5, 5], np.int64)
    assert raw.mvk_chunk_knn_many(one, 9, one, 9, one, one, zero.ctypes.data_as(vp), bad.ctypes.data_as(vp), 2, one, one,
                                  100, 3, one, one, one, 0, None) == -1 and "running sum" in last_error(raw)
    assert raw.mvk_chunk_knn_many(one, 1 << 31, one, 9, one, one, zero.ctypes.data_as(vp), q_off.ctypes.data_as(vp), 2, one,
                                  one, 100, 3, one, one, one, 0, None) == -1

    raw.mvk_chunk_batch_rows.argtypes = [vp, vp, vp, vp, vp, vp, vp, i32, i64, i32, vp, vp, vp]
    assert raw.mvk_chunk_batch_rows(None, None, None, None, None, None, None, 0, 100, 3, None, None, None) == 0
    assert raw.mvk_chunk_batch_rows(None, None, None, None, None, None, None, 4, 0, 3, None, None, None) == 0
    assert raw.mvk_chunk_batch_rows(one, one, one, one, one, one, one, 4, 1 << 31, 3, one, one, None) == -1
    assert raw.mvk_chunk_batch_rows(one, one, one, one, one, one, one, 1 << 12, 1 << 18, 3, one, one, None) == -1
    assert "2^31" in last_error(raw)


def test_wrappers_refuse_cpu_tensors_and_wrong_dtypes():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    i64 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.overlap_pack(torch.zeros(8, 3, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_select_frames(torch.zeros(3, 1, dtype=torch.int32), 8, torch.zeros(8, dtype=torch.int64), i64, i64[:1], i64[:1], 2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_unproject(torch.zeros(1, 2, dtype=torch.int32), torch.zeros(3, 4, 4, dtype=torch.int16),
                            torch.zeros(3, 4, 4, 3), torch.zeros(3, 4, 4), np.eye(3), torch.zeros(1, 4, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_knn_many(torch.zeros(9, 3), i64, i64[:1], i64[:2], [4], torch.zeros(1, 5, 3, dtype=torch.float64),
                           torch.zeros(1, 5, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.chunk_batch_rows(torch.zeros(4, 3), torch.zeros(4, 3, dtype=torch.int64), i64[:2], i64[:1], i64[:1],
                             torch.zeros(2, dtype=torch.int32), i64[:2], 4)
    wsi = mvkpconv.sub("dropin.mvpnet.whole_scene_inputs")
    with pytest.raises(RuntimeError, match="HBM"):
        wsi.SceneFrames({"depth": torch.zeros(3, 4, 4, dtype=torch.int16)})
    with pytest.raises(RuntimeError, match="HBM"):
        next(wsi.group_rgbd_inputs(torch.zeros(9, 3), [i64], [np.zeros(6)], None, 2))
    if torch.cuda.is_available():                             # the dtype checks come after the device check
        with pytest.raises(RuntimeError, match="bool or uint8"):
            ops.overlap_pack(torch.zeros(8, 3, device="cuda"))


def test_new_module_and_signatures():
    import mvkpconv
    wsi = mvkpconv.sub("dropin.mvpnet.whole_scene_inputs")
    wg = mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")
    assert list(inspect.signature(wsi.group_rgbd_inputs).parameters) == [
        "points", "chunk_indices", "chunk_boxes", "scene_frames", "num_rgbd_frames", "k", "chunks_per_forward", "min_nb_pts"]
    assert list(inspect.signature(wsi.predict_whole_scene_rgbd).parameters) == [
        "model", "points", "chunk_indices", "chunk_boxes", "scene_frames", "num_rgbd_frames", "k", "min_nb_pts", "seg_label",
        "evaluator", "num_classes", "chunks_per_forward"]
    p = inspect.signature(wsi.predict_whole_scene_rgbd).parameters
    assert p["k"].default == 3 and p["min_nb_pts"].default == 2048 and p["chunks_per_forward"].default == 1
    assert inspect.isgeneratorfunction(wsi.group_rgbd_inputs) and callable(wg.vote_groups)


# ---------------------------------------------------------------------------------------------------- restatements

@pytest.mark.parametrize("t", [0, 1, 2, 3])
def test_packed_choice_gives_the_references_frames(golden, t):
    g11 = golden("g11_unproject_select")
    table, want = g11["table%d" % t], g11["selected%d" % t].tolist()
    nb, nf = table.shape
    packed = ref.pack_overlap(table)
    assert packed.shape == (nf, (nb + 31) // 32) and packed.dtype == np.uint32
    # every bit where it belongs, nothing past nb
    bits = np.unpackbits(np.ascontiguousarray(packed).view(np.uint8).reshape(nf, -1), axis=1, bitorder="little")
    assert np.array_equal(bits[:, :nb].astype(bool), table.T) and not bits[:, nb:].any()
    everything = ref.pack_mask(np.ones(nb, bool))
    assert ref.select_packed(packed, everything, len(want)) == want == ref.select_frames_table(table, len(want))
    if t == 2:
        assert want[-1] == 0 and want.count(0) == 2                     # this one runs past exhaustion: frame 0 again
    # a chunk that holds every second base point: the packed choice is the table's choice on those rows
    bpi = np.arange(nb, dtype=np.int64) * 3 + 1
    row = bpi[::2].copy()
    assert np.array_equal(ref.base_points_of_chunk(bpi, row), np.arange(nb) % 2 == 0)
    assert ref.select_frames_of_chunk(table, bpi, row, 4) == ref.select_frames_table(table[::2], 4)


def test_packed_choice_on_hand_worked_tables():
    assert ref.select_packed(ref.pack_overlap(np.zeros((70, 5), bool)), ref.pack_mask(np.ones(70, bool)), 3) == [0, 0, 0]
    table = np.zeros((40, 4), bool)
    table[:30, 1] = table[:30, 2] = True                                # two identical columns: the lower index
    table[30:, 3] = True
    everything = ref.pack_mask(np.ones(40, bool))
    assert ref.select_packed(ref.pack_overlap(table), everything, 4) == [1, 3, 0, 0]
    assert ref.select_packed(ref.pack_overlap(table), ref.pack_mask(np.zeros(40, bool)), 2) == [0, 0]   # no base point
    assert ref.select_packed(ref.pack_overlap(table), ref.pack_mask(np.arange(40) >= 30), 2) == [3, 0]
    assert ref.base_points_of_chunk(np.array([5, 9]), np.zeros(0, np.int64)).tolist() == [False, False]
    assert ref.base_points_of_chunk(np.array([2, 5, 9, 11]), np.array([2, 3, 9])).tolist() == [True, False, True, False]


def test_mask_is_strict_and_in_float64():
    bounds = ref.box_bounds([0.0, 1.0, -5.0, 2.0, 3.0, 5.0])
    assert bounds.tolist() == [0.0 - 0.1, 2.0 + 0.1, 1.0 - 0.1, 3.0 + 0.1]
    xyz = np.array([[bounds[0], 2.0, 0.0], [np.nextafter(bounds[0], 1.0), 2.0, 0.0], [1.0, bounds[3], 0.0],
                    [1.0, np.nextafter(bounds[3], 0.0), 0.0], [1.0, 2.0, 0.0]])
    assert ref.pixel_mask(xyz, np.array([True, True, True, True, False]), bounds).tolist() == [False, True, False, True, False]


def test_pad_draws_and_batch_layout():
    sizes, min_nb_pts = [5, 9, 3], 7
    np.random.seed(77)
    extras = ref.pad_extras(sizes, min_nb_pts)
    np.random.seed(77)
    want = [chunk_ref.pad_choice(nc, min_nb_pts) if nc < min_nb_pts else np.arange(nc) for nc in sizes]
    assert all(np.array_equal(np.concatenate([np.arange(nc), e]), w) for nc, e, w in zip(sizes, extras, want))
    rng = np.random.default_rng(1)
    pts = [rng.standard_normal((nc, 3)).astype(np.float32) for nc in sizes]
    knn = [rng.integers(1, 50, size=(nc, 2)) for nc in sizes]
    points, index, lengths = ref.batch_layout(pts, knn, extras)
    assert lengths.tolist() == [7, 9, 7] and points.shape == (3, 3, 9) and index.shape == (3, 9, 2)
    for g in range(3):
        assert np.array_equal(points[g, :, :lengths[g]], pts[g][want[g]].T) and not points[g, :, lengths[g]:].any()
        assert np.array_equal(index[g, :lengths[g]], knn[g][want[g]]) and not index[g, lengths[g]:].any()
