"""CPU-only: the library's side of the training inputs (include/mvkpconv_train.h parsed and bound beside the first two
headers, whose tables stay what they were; size refusals and empty problems through raw ctypes; wrappers that refuse CPU
tensors) and the NumPy restatements of tests/train_inputs_ref.py: against the reference's own __getitem__ (fixture g12,
tests/golden/make_g12_train_chunks.py), the resample rule's properties, mix32 against hand-computed values."""
import ctypes
import inspect
import re

import numpy as np
import pytest

import train_inputs_ref as ref

TRAIN_EXPORTS = ("mvk_train_chunk_pick", "mvk_train_chunk_resample", "mvk_train_select_frames", "mvk_train_unproject",
                 "mvk_train_batch_rows")
SCENE_EXPORTS = ("mvk_overlap_pack", "mvk_chunk_select_frames", "mvk_chunk_unproject", "mvk_scene_inputs_workspace",
                 "mvk_chunk_knn_many", "mvk_chunk_batch_rows")
CASES = ("c0", "c1", "c2", "c3")


@pytest.fixture(scope="module")
def L():
    import mvkpconv
    return mvkpconv.sub("_lib")


@pytest.fixture(scope="module")
def g12(golden):
    return golden("g12_train_chunks")


def case_of(g12, name):
    return {key[len(name) + 1:]: v for key, v in g12.items() if key.startswith(name + "/")}


def host_scene(c):
    return {"points": c["points"], "seg_label": c["seg_label"], "base_point_ind": c["base_point_ind"],
            "pointwise_rgbd_overlap": c["overlap"], "depth": c["depth"], "images": c["images"], "poses": c["poses"],
            "cam_matrix": c["cam_matrix"]}


def rotation_of(angle):
    from scipy.spatial.transform import Rotation
    return None if np.isnan(angle) else Rotation.from_euler("z", float(angle), degrees=True).as_matrix()


# ------------------------------------------------------------------------------------------------------------ binding

def test_third_header_parses_and_leaves_the_first_two_alone(L):
    import mvkpconv
    text = open(mvkpconv._ROOT + "/include/mvkpconv_train.h").read()
    functions, structs, constants = L.parse_header(text)
    assert tuple(functions) == TRAIN_EXPORTS == tuple(L.TRAIN_FUNCTIONS) and structs == {}
    assert constants == L.TRAIN_CONSTANTS == {"MVK_TRAIN_MAX_TRIES": 32, "MVK_TRAIN_PICK_TILE": 1024,
                                              "MVK_TRAIN_RESAMPLE_STRIDE": 1024}
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#ifndef MVKPCONV_TRAIN_H" in code and "MVK_ABI_VERSION" not in code and code.count('extern "C"') == 1
    assert "struct" not in code
    for name, (ret, params) in functions.items():
        assert params[-1] == ("void*", "stream") and ret == "int", name
    # the first two headers' tables are what they were
    assert len(L.FUNCTIONS) == len(L.EXPORTS) == 133 and len(L.STRUCTS) == 6 and len(L.CONSTANTS) == 9 and L.ABI_VERSION == 9
    assert tuple(L.SCENE_FUNCTIONS) == SCENE_EXPORTS
    assert L.SCENE_CONSTANTS == {"MVK_SCENE_MAX_BASE": 524288, "MVK_SCENE_MAX_FRAMES": 4096}
    assert not set(TRAIN_EXPORTS) & (set(L.EXPORTS) | set(SCENE_EXPORTS))


def test_train_functions_are_exported_and_bound(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    assert lib.mvk_abi_version() == 9
    for name in TRAIN_EXPORTS:
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(L.TRAIN_FUNCTIONS[name][1]) and fn.restype is ctypes.c_int


def last_error(raw):
    raw.mvk_last_error.restype = ctypes.c_char_p
    return raw.mvk_last_error().decode()


def test_size_refusals_and_empty_problems_through_raw_ctypes(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    i64, i32, f32, f64, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_void_p
    one = ctypes.c_void_p(64)                                 # a non-null address that must never be touched
    big = 1 << 31

    pick = raw.mvk_train_chunk_pick
    pick.argtypes = [vp, vp, i64, vp, i32, i64, i64, i64, vp, vp, i32, i32, f32, f32, f32, f32, f64, i64, vp, i64, vp, vp,
                     vp, vp, vp, vp, vp]

    def call_pick(P=100, S=1, B=1, T=10, max_points=100, total=100, p=one):
        return pick(p, p, P, p, S, 10, 5, 10, p, p, B, T, 1.5, 1.5, 0.2, 0.2, 0.3, max_points, p, total, p, p, p, p, p, p, None)

    assert call_pick(B=0, p=None) == 0                        # no item: nothing is launched, nothing is touched
    assert call_pick(P=big) == -1 and "2^31" in last_error(raw)
    assert call_pick(total=big) == -1 and call_pick(max_points=big) == -1 and call_pick(B=-1) == -1
    assert call_pick(T=33) == -1 and "32" in last_error(raw)
    assert call_pick(B=1 << 20, max_points=1 << 22) == -1     # the grid
    assert call_pick(p=None) == -1 and "null" in last_error(raw)

    rs = raw.mvk_train_chunk_resample
    rs.argtypes = [vp, i64, vp, vp, vp, i32, i64, i32, vp, vp, vp]
    assert rs(None, 0, None, None, None, 0, 256, 32, None, None, None) == 0
    assert rs(None, 0, None, None, None, 4, 0, 32, None, None, None) == 0
    assert rs(one, 10, one, one, one, 4, 256, 0, one, one, None) == -1 and "key_bits" in last_error(raw)
    assert rs(one, 10, one, one, one, 4, 256, 33, one, one, None) == -1
    assert rs(one, big, one, one, one, 4, 256, 32, one, one, None) == -1 and "2^31" in last_error(raw)
    assert rs(one, 10, one, one, one, 1 << 16, 1 << 16, 32, one, one, None) == -1
    assert rs(one, 10, one, one, one, 4, big, 32, one, one, None) == -1

    sf = raw.mvk_train_select_frames
    sf.argtypes = [vp, i64, vp, i64, vp, i32, i64, i64, vp, vp, i64, vp, vp, i32, i32, i64, i64, vp, vp]
    assert sf(None, 0, None, 0, None, 1, 10, 5, None, None, 0, None, None, 0, 3, 10, 5, None, None) == 0       # no item
    assert sf(None, 0, None, 0, None, 1, 10, 5, None, None, 0, None, None, 4, 0, 10, 5, None, None) == 0       # no round
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, 10, one, one, 1, 3, 524289, 5, one, None) == -1
    assert "524288" in last_error(raw) and "no fallback" in last_error(raw)
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, 10, one, one, 1, 3, 10, 4097, one, None) == -1
    assert "4096" in last_error(raw)
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, big, one, one, 1, 3, 10, 5, one, None) == -1

    up = raw.mvk_train_unproject
    up.argtypes = [vp, vp, i32, i32, vp, i32, i64, i64, i64, i64, vp, vp, vp, vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    assert up(None, None, 0, 3, None, 1, 10, 10, 5, 10, None, None, None, None, 12, 16, None, None, None, None, None, None,
              None, None, None) == 0
    assert up(one, one, 4, 3, one, 1, 10, 10, 5, 10, one, one, one, one, 1 << 15, 1 << 15, one, None, None, one, one, one,
              one, one, None) == -1 and "2^31" in last_error(raw)
    assert up(one, one, -1, 3, one, 1, 10, 10, 5, 10, one, one, one, one, 12, 16, one, None, None, one, one, one, one, one,
              None) == -1

    br = raw.mvk_train_batch_rows
    br.argtypes = [vp, vp, i64, vp, vp, i32, i64, vp, vp, vp]
    assert br(None, None, 10, None, None, 0, 256, None, None, None) == 0
    assert br(None, None, 10, None, None, 4, 0, None, None, None) == 0
    assert br(one, one, 10, one, None, 4, big, one, one, None) == -1
    assert br(one, one, 10, one, None, 1 << 12, 1 << 18, one, one, None) == -1 and "2^31" in last_error(raw)
    assert br(one, one, big, one, None, 4, 256, one, one, None) == -1


def test_wrappers_refuse_cpu_tensors():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    ti = mvkpconv.sub("dropin.mvpnet.train_inputs")
    i64 = torch.zeros(4, dtype=torch.int64)
    table = np.array([[0, 9, 0, 8, 0, 3, 0, 0]], np.int64)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.TrainResident(torch.zeros(9, 3), torch.zeros(9, dtype=torch.int64), torch.zeros(8, dtype=torch.int64),
                          torch.zeros(3, dtype=torch.int32), torch.zeros(3, 4, 4, dtype=torch.int16), torch.zeros(3, 4, 4, 3),
                          torch.zeros(3, 4, 4), torch.zeros(1, 9, dtype=torch.float64), table)
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.train_chunk_pick(None, i64[:1], i64.view(1, 4), i64[:1], 9)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.train_chunk_resample(i64, i64[:1], i64[:1], i64[:1], 2)
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.train_select_frames(None, i64[:1], i64, i64[:1], i64[:1], 2)
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.train_unproject(None, torch.zeros(1, 2, dtype=torch.int32), i64[:1], torch.zeros(1, 4))
    with pytest.raises(RuntimeError, match="HBM"):
        ops.train_batch_rows(torch.zeros(4, 3), i64, i64.view(1, 4))
    with pytest.raises(RuntimeError, match="HBM"):
        ti.TrainScenes([{"depth": torch.zeros(3, 4, 4, dtype=torch.int16)}])
    with pytest.raises(ValueError, match="at least one scene"):
        ti.TrainScenes([])


def test_new_module_and_signatures():
    import mvkpconv
    ti = mvkpconv.sub("dropin.mvpnet.train_inputs")
    p = inspect.signature(ti.train_chunk_batch).parameters
    assert list(p)[:11] == ["scenes", "scene_ids", "nb_pts", "num_rgbd_frames", "k", "chunk_size", "chunk_thresh",
                            "chunk_margin", "flip", "z_rot", "tries"]
    assert (p["k"].default, p["chunk_size"].default, p["chunk_thresh"].default, p["chunk_margin"].default) == \
        (3, (1.5, 1.5), 0.3, (0.2, 0.2))
    assert (p["flip"].default, p["z_rot"].default, p["tries"].default, p["key_bits"].default) == (0.0, None, 10, 32)
    doc = ti.__doc__
    assert "Colour jitter" in doc and "ASCENDING" in doc and "stream" in doc


def test_draw_order_of_the_host_is_the_documented_one():
    import mvkpconv
    ti = mvkpconv.sub("dropin.mvpnet.train_inputs")
    np.random.seed(11)
    centers, seeds, flips, angles = ti.draw_items([50, 70], 2, flip=0.5, z_rot=(-180, 180), tries=10)
    np.random.seed(11)
    for b, n in enumerate([50, 70]):
        assert np.array_equal(centers[b], np.random.randint(n, size=10))
        assert seeds[b] == np.random.randint(2 ** 63, dtype=np.int64)
        assert np.array_equal(flips[b], np.random.rand(2) < 0.5)
        assert angles[b] == np.random.uniform(low=-180, high=180)
    assert ti.draw_items([5], 2)[2:] == (None, None)
    m = ti.z_rotation(30.0)
    c, s = np.cos(np.pi / 6), np.sin(np.pi / 6)
    assert m.dtype == np.float64 and np.allclose(m, [[c, -s, 0], [s, c, 0], [0, 0, 1]], atol=1e-15)


# ------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("name", CASES)
def test_restatement_fed_the_recorded_draws_gives_the_references_item(g12, name):
    c = case_of(g12, name)
    nb_pts, nv, k = int(g12["nb_pts"]), int(g12["nv"]), int(g12["k"])
    got = ref.item(host_scene(c), c["centers"], nb_pts, nv, k, choice=c["choice"], flips=c["flips"],
                   rot=rotation_of(c["angle"][0]))
    for key in ("points", "seg_label", "images", "image_mask", "knn_indices"):
        want = c["out_" + key]
        assert got[key].dtype == want.dtype and got[key].shape == want.shape and np.array_equal(got[key], want), key
    assert got["chunk_try"] == int(c["chunk_try"][0]) and np.array_equal(got["row"], c["row"])
    assert got["box"].dtype == np.float32 and np.array_equal(got["box"], c["box"])
    # image_xyz: the reference's BLAS products and csrc/unproject.h's written order are different float64 evaluations of
    # one expression. Each is within a few float64 ulp of the exact value, so their float32 roundings differ by at most
    # one float32 ulp, and one more after the float64 rotation of two such values: 2 ulp of the largest coordinate
    # (measured on this fixture: no value differs)
    want = c["out_image_xyz"]
    assert got["image_xyz"].dtype == want.dtype == np.float32 and got["image_xyz"].shape == want.shape
    diff = np.abs(got["image_xyz"].astype(np.float64) - want.astype(np.float64)).max()
    bound = 2.0 * float(np.spacing(np.float32(np.abs(want).max())))
    print("%s: image_xyz differs from the reference by at most %.3g (bound %.3g)" % (name, diff, bound))
    assert diff <= bound


def test_fixture_holds_its_four_cases(g12):
    nb_pts = int(g12["nb_pts"])
    tries = {name: int(case_of(g12, name)["chunk_try"][0]) for name in CASES}
    sizes = {name: len(case_of(g12, name)["row"]) for name in CASES}
    assert tries["c0"] == 0 and sizes["c0"] > nb_pts                    # more points than nb_pts
    assert tries["c1"] >= 0 and sizes["c1"] < nb_pts                    # fewer: the pad branch
    c1 = case_of(g12, "c1")
    assert np.array_equal(c1["choice"][:sizes["c1"]], np.arange(sizes["c1"])) and (c1["choice"] < sizes["c1"]).all()
    c2 = case_of(g12, "c2")
    counts = ref.crop(c2["points"], c2["seg_label"], c2["centers"])[0]
    assert tries["c2"] > 0 and counts[0, 0] > 0 and counts[0, 1] / counts[0, 0] < 0.3    # a first try that fails
    assert tries["c3"] == -1 and sizes["c3"] == len(case_of(g12, "c3")["points"])        # the whole scene
    assert case_of(g12, "c0")["flips"].any() and not np.isnan(case_of(g12, "c0")["angle"][0])


# ------------------------------------------------------------------------------------------------- the resample rule

def step_by_step(x):
    """mix32 on a Python integer."""
    x ^= x >> 16
    x = (x * 0x7feb352d) % (1 << 32)
    x ^= x >> 15
    x = (x * 0x846ca68b) % (1 << 32)
    return x ^ (x >> 16)


def test_mix32_against_hand_computed_values():
    # worked by hand for x = 1:  1 ^ (1 >> 16) = 1;  1 * 0x7feb352d = 0x7feb352d;  0x7feb352d >> 15 = 0xffd6,
    # 0x7feb352d ^ 0xffd6 = 0x7febcafb;  0x7febcafb * 0x846ca68b mod 2^32 = 0x6889f849;  0x6889f849 >> 16 = 0x6889,
    # 0x6889f849 ^ 0x6889 = 0x688990c0. The other two the same way; 0 stays 0 (every step maps 0 to 0).
    values = {0: 0, 1: 0x688990c0, 0xdeadbeef: 0xe628c683, 0xffffffff: 0x6768824a}
    got = ref.mix32(np.array(list(values), np.uint64))
    assert got.dtype == np.uint64 and [int(v) for v in got] == list(values.values())
    assert all(step_by_step(x) == want for x, want in values.items())
    # draw(i) composes two of them: seed = hi << 32 | lo
    seed, i = (7 << 32) | 9, 5
    assert int(ref.draw(seed, np.array([i]))[0]) == step_by_step(9 ^ step_by_step((7 + i * 0x9e3779b9) % (1 << 32)))
    # a negative int64 seed is its two's complement; key() keeps the top bits
    assert int(ref.draw(-1, np.array([0]))[0]) == step_by_step(0xffffffff ^ step_by_step(0xffffffff))
    assert np.array_equal(ref.keys_of(seed, 9, 4), ref.draw(seed, np.arange(9)) >> np.uint64(28))


@pytest.mark.parametrize("key_bits", [4, 32])
@pytest.mark.parametrize("nc", [256, 257, 1023, 1024, 1025, 5000])
def test_resample_takes_exactly_nb_pts_distinct_positions_ascending(nc, key_bits):
    nb_pts = 256
    pos = ref.resample_positions(nc, nb_pts, seed=1234567 + nc, key_bits=key_bits)
    assert pos.dtype == np.int64 and len(pos) == nb_pts == len(np.unique(pos))
    assert (np.diff(pos) > 0).all() and pos[0] >= 0 and pos[-1] < nc
    # the order (key, position): every taken key <= every left key, and among the threshold's equals the first positions
    keys = ref.keys_of(1234567 + nc, nc, key_bits)
    taken = np.zeros(nc, bool)
    taken[pos] = True
    if nc > nb_pts:
        thr = keys[taken].max()
        assert thr <= keys[~taken].min()
        equal = np.nonzero(keys == thr)[0]
        n_taken = int(taken[equal].sum())
        assert taken[equal[:n_taken]].all() and not taken[equal[n_taken:]].any()
        if key_bits == 4:
            assert n_taken < len(equal)                                 # a tie at the threshold really occurs


@pytest.mark.parametrize("nc", [1, 7, 255])
def test_resample_pads_a_short_row_within_it(nc):
    nb_pts = 256
    pos = ref.resample_positions(nc, nb_pts, seed=-99, key_bits=32)
    assert np.array_equal(pos[:nc], np.arange(nc)) and (pos[nc:] >= 0).all() and (pos[nc:] < nc).all()
    want = (ref.draw(-99, nc + np.arange(nb_pts - nc)) * np.uint64(nc)) >> np.uint64(32)
    assert np.array_equal(pos[nc:], want.astype(np.int64))
    if nc == 255:
        assert ref.resample_positions(0, 4, 1).tolist() == [-1] * 4


def test_resample_subset_is_close_to_uniform():
    # every position of a row of 40 is taken about 10 / 40 of the time over 2000 seeds (a hash, not a proof: 5 sigma)
    hits = np.zeros(40)
    for seed in range(2000):
        hits[ref.resample_positions(40, 10, seed * 7919 + 1)] += 1
    sigma = np.sqrt(2000 * 0.25 * 0.75)
    assert np.abs(hits - 500).max() < 5 * sigma
