"""CPU-only: the library's side of the sphere batches (include/mvkpconv_sphere.h parsed and bound beside the other three
headers, whose tables stay what they were; size refusals and empty problems through raw ctypes; wrappers that refuse CPU
tensors; the host's draw order and its augmentation matrices) and the NumPy restatement of tests/sphere_inputs_ref.py
against the reference's own potential_item (fixture g18, tests/golden/make_g18_sphere_batch.py) and against a plain
brute-force k-NN."""
import ctypes
import hashlib
import inspect
import re

import numpy as np
import pytest

import sphere_inputs_ref as ref

SPHERE_EXPORTS = ("mvk_knn_ragged_workspace", "mvk_knn_f64_ragged", "mvk_sphere_pick", "mvk_sphere_members",
                  "mvk_sphere_select_frames", "mvk_sphere_batch_rows")
TRAIN_EXPORTS = ("mvk_train_chunk_pick", "mvk_train_chunk_resample", "mvk_train_select_frames", "mvk_train_unproject",
                 "mvk_train_batch_rows")
SCENE_EXPORTS = ("mvk_overlap_pack", "mvk_chunk_select_frames", "mvk_chunk_unproject", "mvk_scene_inputs_workspace",
                 "mvk_chunk_knn_many", "mvk_chunk_batch_rows")
# the other three headers stay byte for byte what they were
HEADER_SHA256 = {"mvkpconv.h": "9808f0a60d4498f033dc5ea4e52b827d0ed9da74cd15c61ccf035f0cfdf73c37",
                 "mvkpconv_scene.h": "92af2ba9aa55165458774c55c5895d26d9337a88298186ef972e337f943bfca6",
                 "mvkpconv_train.h": "3e7ec841414a9980878f6e60886dbcbc3d99767226a9151b67c72ce9602a0534"}
CASES = ("stop2", "stop3")


@pytest.fixture(scope="module")
def L():
    import mvkpconv
    return mvkpconv.sub("_lib")


@pytest.fixture(scope="module")
def g18(golden):
    return golden("g18_sphere_batch")


class Npz(dict):
    files = property(lambda self: list(self))


# ------------------------------------------------------------------------------------------------------------ binding

def test_fourth_header_parses_and_leaves_the_other_three_alone(L):
    import mvkpconv
    text = open(mvkpconv._ROOT + "/include/mvkpconv_sphere.h").read()
    functions, structs, constants = L.parse_header(text)
    assert tuple(functions) == SPHERE_EXPORTS == tuple(L.SPHERE_FUNCTIONS) and structs == {}
    assert constants == L.SPHERE_CONSTANTS == {"MVK_KNN_RAGGED_MAX_ITEMS": 1024, "MVK_SPHERE_TILE": 1024,
                                               "MVK_SPHERE_MAX_SLOTS": 1024}
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert "#ifndef MVKPCONV_SPHERE_H" in code and "MVK_ABI_VERSION" not in code and code.count('extern "C"') == 1
    assert "struct" not in code and "mvkpconv" not in code.replace("MVKPCONV_SPHERE_H", "")
    for name, (ret, params) in functions.items():
        if name == "mvk_knn_ragged_workspace":
            assert ret == "int64_t"
        else:
            assert params[-1] == ("void*", "stream") and ret == "int", name
    for name, digest in HEADER_SHA256.items():
        assert hashlib.sha256(open(mvkpconv._ROOT + "/include/" + name, "rb").read()).hexdigest() == digest, name
    assert len(L.FUNCTIONS) == len(L.EXPORTS) == 133 and len(L.STRUCTS) == 6 and len(L.CONSTANTS) == 9 and L.ABI_VERSION == 9
    assert tuple(L.SCENE_FUNCTIONS) == SCENE_EXPORTS and tuple(L.TRAIN_FUNCTIONS) == TRAIN_EXPORTS
    assert L.SCENE_CONSTANTS == {"MVK_SCENE_MAX_BASE": 524288, "MVK_SCENE_MAX_FRAMES": 4096}
    assert L.TRAIN_CONSTANTS == {"MVK_TRAIN_MAX_TRIES": 32, "MVK_TRAIN_PICK_TILE": 1024, "MVK_TRAIN_RESAMPLE_STRIDE": 1024}
    assert not set(SPHERE_EXPORTS) & (set(L.EXPORTS) | set(SCENE_EXPORTS) | set(TRAIN_EXPORTS))


def test_sphere_functions_are_exported_and_bound(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    lib = L.lib()
    assert lib.mvk_abi_version() == 9
    for name in SPHERE_EXPORTS:
        assert hasattr(raw, name)
        fn = getattr(lib, name)
        assert len(fn.argtypes) == len(L.SPHERE_FUNCTIONS[name][1])
        assert fn.restype is (ctypes.c_int64 if name == "mvk_knn_ragged_workspace" else ctypes.c_int)


def last_error(raw):
    raw.mvk_last_error.restype = ctypes.c_char_p
    return raw.mvk_last_error().decode()


def test_size_refusals_and_empty_problems_through_raw_ctypes(L):
    raw = ctypes.CDLL(L.LIB_PATH)
    i64, i32, f64, vp = ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_void_p
    one = ctypes.c_void_p(64)                                 # a non-null address that must never be touched
    big = 1 << 31

    wsz = raw.mvk_knn_ragged_workspace
    wsz.argtypes, wsz.restype = [i32, i64, i64, i32], i64
    assert wsz(5, 20000, 96000, 3) > 5 * 96000 * 28 and wsz(1, 0, 0, 1) > 0
    assert wsz(0, 10, 10, 3) == -1 and wsz(1025, 10, 10, 3) == -1 and wsz(1, 10, 10, 0) == -1 and wsz(1, 10, 10, 9) == -1
    assert wsz(4, 1 << 29, 1 << 27, 3) == -1 and wsz(1, -1, 10, 3) == -1

    knn = raw.mvk_knn_f64_ragged
    knn.argtypes = [vp, i64, vp, i64, vp, i32, vp, vp, i64, i32, vp, vp, vp, i64, vp]
    assert knn(None, 0, None, 0, None, 3, None, None, 64, 3, None, None, None, 0, None) == 0          # no slot
    assert knn(None, 0, None, 10, None, 0, None, None, 64, 3, None, None, None, 0, None) == 0         # no item
    assert knn(one, 9, one, 10, one, 2, one, one, 64, 9, one, None, one, 1 << 30, None) == -1 and "k=9" in last_error(raw)
    assert knn(one, 9, one, 10, one, 2, one, one, 64, 0, one, None, one, 1 << 30, None) == -1
    assert knn(one, 9, one, 10, one, 1025, one, one, 64, 3, one, None, one, 1 << 40, None) == -1 and "1024" in last_error(raw)
    assert knn(one, 9, one, 1 << 29, one, 4, one, one, 1 << 27, 3, one, None, one, 1 << 40, None) == -1
    assert "2^30" in last_error(raw)
    assert knn(one, 9, one, 10, one, 2, one, one, 64, 3, one, None, one, 16, None) == -1 and "workspace" in last_error(raw)
    assert knn(None, 9, one, 10, one, 2, one, one, 64, 3, one, None, one, 1 << 30, None) == -1 and "null" in last_error(raw)
    assert knn(one, 9, one, -1, one, 2, one, one, 64, 3, one, None, one, 1 << 30, None) == -1

    pick = raw.mvk_sphere_pick
    pick.argtypes = [vp, i64, vp, vp, vp, vp, vp, i64, vp, i32, i64, i64, i64, f64, i64, i32, vp, vp, vp, vp, vp, vp]

    def call_pick(PP=50, P=100, S=1, radius=0.8, B=2, p=one):
        return pick(p, PP, p, p, p, p, p, P, p, S, 10, 5, 10, radius, 1000, B, p, p, p, p, p, None)

    assert call_pick(B=0, p=None) == 0
    assert call_pick(PP=big) == -1 and "2^31" in last_error(raw)
    assert call_pick(P=big) == -1 and call_pick(B=-1) == -1 and call_pick(B=1025) == -1
    assert call_pick(radius=0.0) == -1 and "in_radius" in last_error(raw)
    assert call_pick(p=None) == -1 and "null" in last_error(raw)

    mem = raw.mvk_sphere_members
    mem.argtypes = [vp, i64, vp, i32, i64, i64, i64, vp, vp, i32, f64, i64, i64, vp, vp, vp, vp, vp]

    def call_mem(P=100, B=2, radius=0.8, max_points=100, cap=50, p=one):
        return mem(p, P, p, 1, 10, 5, 10, p, p, B, radius, max_points, cap, p, p, p, p, None)

    assert call_mem(B=0, p=None) == 0
    assert call_mem(P=big) == -1 and call_mem(cap=big) == -1 and call_mem(max_points=big) == -1 and "2^31" in last_error(raw)
    assert call_mem(radius=-1.0) == -1 and call_mem(B=1025) == -1
    assert call_mem(p=None) == -1 and "null" in last_error(raw)

    sf = raw.mvk_sphere_select_frames
    sf.argtypes = [vp, i64, vp, i64, vp, i32, i64, i64, vp, vp, i64, vp, i32, i32, i64, i64, vp, vp]
    assert sf(None, 0, None, 0, None, 1, 10, 5, None, None, 0, None, 0, 3, 10, 5, None, None) == 0            # no slot
    assert sf(None, 0, None, 0, None, 1, 10, 5, None, None, 0, None, 4, 0, 10, 5, None, None) == 0            # no round
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, 10, one, 1, 3, 524289, 5, one, None) == -1
    assert "524288" in last_error(raw) and "no fallback" in last_error(raw)
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, 10, one, 1, 3, 10, 4097, one, None) == -1 and "4096" in last_error(raw)
    assert sf(one, 10, one, 10, one, 1, 10, 5, one, one, big, one, 1, 3, 10, 5, one, None) == -1
    assert sf(one, 10, one, 10, one, 1, 10, 5, None, one, 10, one, 1, 3, 10, 5, one, None) == -1 and "null" in last_error(raw)

    br = raw.mvk_sphere_batch_rows
    br.argtypes = [vp, vp, vp, i64, vp, i32, i64, i64, i64, vp, vp, vp, i64, vp, i32, vp, vp, vp, vp, vp, i32, i64] + [vp] * 8

    def call_br(P=100, cap=50, B=2, k=3, npix=576, p=one):
        return br(p, p, p, P, p, 1, 10, 5, 10, p, p, p, cap, p, B, p, p, None, p, p, k, npix, p, p, p, p, p, p, p, None)

    assert call_br(cap=0, p=None) == 0
    assert call_br(k=9) == -1 and call_br(B=1025) == -1 and call_br(P=big) == -1 and call_br(npix=big) == -1
    assert call_br(cap=big) == -1 and "bad sizes" in last_error(raw)
    assert call_br(p=None) == -1 and "null" in last_error(raw)


def test_wrappers_refuse_cpu_tensors():
    import torch
    import mvkpconv
    ops = mvkpconv.sub("ops")
    si = mvkpconv.sub("dropin.datasets.sphere_inputs")
    i64 = torch.zeros(4, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.knn_f64_ragged(torch.zeros(4, 3), i64, i64[:2], torch.zeros(1, 4, 3, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.SphereResident(None, torch.zeros(4, 3), torch.zeros(4, 3), torch.zeros(4, dtype=torch.float64), np.zeros((1, 2)))
    with pytest.raises(RuntimeError, match="SphereResident"):
        ops.sphere_pick(None, 0.8, 100, 2)
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.sphere_members(None, i64[:2], torch.zeros(2, 3), 0.8, 10)
    with pytest.raises(RuntimeError, match="TrainResident"):
        ops.sphere_select_frames(None, i64[:2], i64, i64[:3], 2)
    with pytest.raises(RuntimeError, match="SphereResident"):
        ops.sphere_batch_rows(None, i64[:2], torch.zeros(2, 3), i64, i64[:3], None, None, None, None, 10)
    with pytest.raises(RuntimeError, match="HBM"):
        si.SphereScenes([{"depth": torch.zeros(3, 4, 4, dtype=torch.int16)}], 0.8)
    with pytest.raises(ValueError, match="at least one scene"):
        si.SphereScenes([], 0.8)


def test_new_module_and_signatures():
    import mvkpconv
    si = mvkpconv.sub("dropin.datasets.sphere_inputs")
    p = inspect.signature(si.sphere_batch).parameters
    assert list(p)[:9] == ["scenes", "config", "max_spheres", "batch_limit", "cap", "num_rgbd_frames", "k", "flip", "noise"]
    assert (p["k"].default, p["flip"].default, p["noise"].default) == (3, 0.0, None)
    p = inspect.signature(si.SphereScenes.__init__).parameters
    assert list(p)[1:] == ["scene_dicts", "in_radius", "mask_margin", "init_potentials"] and p["mask_margin"].default == 0.1
    assert list(inspect.signature(si.to_sphere_batch).parameters)[:3] == ["out", "config", "limits"]
    doc = si.__doc__
    assert "Colour jitter" in doc and "ASCENDING" in doc and "noise" in doc and "up front" in doc


class DrawCfg(object):
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min, augment_scale_max = 0.9, 1.1
    augment_symmetries = [True, False, True]
    augment_color = 0.7


def test_draw_order_and_augmentation_of_the_host():
    """draw_spheres draws slot by slot in the documented order; augmentation_of equals the restatement's matrices for
    'vertical', 'all' (through the drop-in's create_3D_rotations), 'none', and both scale forms."""
    import mvkpconv
    si = mvkpconv.sub("dropin.datasets.sphere_inputs")
    kp = mvkpconv.sub("dropin.kernels.kernel_points")
    np.random.seed(11)
    draws = si.draw_spheres(DrawCfg, 2, 3, flip=0.5)
    np.random.seed(11)
    for d in draws:
        assert np.array_equal(d["flip"], np.random.rand(3) < 0.5)
        assert d["rot"] == [np.random.rand()]
        assert np.array_equal(d["scale"], np.random.rand(3))
        assert np.array_equal(d["sym"], np.random.randint(2, size=3))
        assert d["keep_color"] == (not (np.random.rand() > 0.7))
    assert si.draw_spheres(DrawCfg, 1, 3)[0]["flip"] is None
    for rotation, aniso in (("vertical", True), ("all", False), ("none", True)):
        cfg = type("C", (DrawCfg,), dict(augment_rotation=rotation, augment_scale_anisotropic=aniso))
        np.random.seed(5)
        d = si.draw_spheres(cfg, 1, 3)[0]
        assert len(d["rot"]) == {"vertical": 1, "all": 3, "none": 0}[rotation] and np.ndim(d["scale"]) == int(aniso)
        R, scale = si.augmentation_of(cfg, d)
        R2, scale2 = ref.augment_params(cfg, d, kp.create_3D_rotations)
        assert R.dtype == scale.dtype == np.float32 and R.shape == (3, 3) and scale.shape == (3,)
        assert np.array_equal(R, R2) and np.array_equal(scale, scale2)
        if rotation == "vertical":
            th = d["rot"][0] * 2 * np.pi
            assert np.array_equal(R, np.array([[np.cos(th), -np.sin(th), 0], [np.sin(th), np.cos(th), 0], [0, 0, 1]], np.float32))
        if rotation == "all":
            assert np.allclose(R @ R.T, np.eye(3), atol=1e-6)
            want = (float(d["scale"]) * (1.1 - 0.9) - 0.9) * (1 - np.array([1, 0, 1]) * d["sym"] * 2)      # '- min_s', as written
            assert np.array_equal(scale, want.astype(np.float32))


def test_features_follow_every_branch():
    import torch
    import mvkpconv
    si = mvkpconv.sub("dropin.datasets.sphere_inputs")
    rng = np.random.default_rng(0)
    colors, world = rng.random((7, 3)).astype(np.float32), rng.random((7, 3)).astype(np.float32)
    cases = [(dict(late_fusion=True, in_features_dim=d), w) for d, w in ((1, 1), (2, 2), (4, 4), (7, 7))]
    cases += [(dict(middle_fusion=True, in_features_dim_3d=d, in_features_dim=99), w) for d, w in ((1, 1), (2, 2), (4, 4), (7, 7))]
    cases += [(dict(early_fusion=True, in_features_dim=d), w) for d, w in ((65, 1), (66, 2), (68, 4), (69, 5), (71, 7))]
    cases += [(dict(in_features_dim=2), 2)]
    for attrs, width in cases:
        cfg = type("C", (), attrs)
        for upc in (False, True):
            want = ref.features(cfg, colors, world, upc)
            got = si.stacked_3d_features(cfg, torch.from_numpy(colors), torch.from_numpy(world), upc).numpy()
            assert want.shape == (7, width) and np.array_equal(got, want), (attrs, upc)
    z = ref.features(type("C", (), dict(early_fusion=True, in_features_dim=66)), colors, world)
    assert np.array_equal(z[:, 0], np.ones(7, np.float32)) and np.array_equal(z[:, 1], world[:, 2])
    rgb = ref.features(type("C", (), dict(early_fusion=True, in_features_dim=68)), colors, world, True)
    assert np.array_equal(rgb[:, 1:], colors)
    for f in (lambda c: ref.features(c, colors, world),
              lambda c: si.stacked_3d_features(c, torch.from_numpy(colors), torch.from_numpy(world))):
        with pytest.raises(ValueError, match="choose one fusion"):
            f(type("C", (), dict(early_fusion=True, in_features_dim=67)))


# ------------------------------------------------------------------------------------------- against the reference

@pytest.mark.parametrize("name", CASES)
def test_restatement_fed_the_logged_draws_gives_the_references_batch(g18, name):
    """stacked_points, features, labels, input_inds, cloud_inds, point_inds, images, image_mask, knn, scales and rots of the
    reference's own potential_item, exactly. The index ORDER inside a sphere is ascending here and the KD-tree's there:
    both are compared after sorting by input_inds (ref.compare_with_golden). The potentials afterwards are the
    reference's bit for bit."""
    g = ref.golden_case(Npz(g18), name)
    pots = [p.copy() for p in g["potentials"]]
    mine = ref.sphere_batch(g["scenes"], pots, g["config"], g["max_spheres"], int(g["batch_limit"]), g["nv"], g["draws"],
                            k=g["k"], noise=ref.golden_noise_rows(g))
    worst = ref.compare_with_golden(mine, g)
    assert worst <= 2.0                                # image_xyz: DESIGN.md 7q's bound, in ulp of the largest coordinate
    for i, p in enumerate(pots):
        assert np.array_equal(p, g["potentials_after%d" % i])
    # one sphere more than the reference made is allowed: the stop rule ends the batch where it did
    more = ref.sphere_batch(g["scenes"], [p.copy() for p in g["potentials"]], g["config"], g["max_spheres"] + 2,
                            int(g["batch_limit"]), g["nv"], g["draws"] + g["draws"][:2], k=g["k"], noise=ref.golden_noise_rows(g))
    assert more["num_spheres"] == g["max_spheres"]


def test_fixture_holds_its_cases(g18):
    """Two scenes within the fixture's size limits; batches that stop on batch_limit with the second and the third sphere;
    a flipped and an unflipped view, the symmetry applied and not, a dropped and a kept colour in each."""
    assert int(g18["num_scenes"]) == 2 and int(g18["nv"]) == 3 and int(g18["k"]) == 3
    for i in range(2):
        assert len(g18["scene%d/points" % i]) <= 3000 and g18["scene%d/depth" % i].shape == (12, 12, 16)
        assert len(g18["scene%d/base_point_ind" % i]) == 200
    for name, n in (("stop2", 2), ("stop3", 3)):
        g = ref.golden_case(Npz(g18), name)
        lens = g["stack_lengths"]
        assert len(lens) == n and lens[:-1].sum() <= int(g["batch_limit"]) < lens.sum()
        flips = np.stack([d["flip"] for d in g["draws"]])
        assert flips.any() and not flips.all()
        assert {int(d["sym"][0]) for d in g["draws"]} == {0, 1} and {d["keep_color"] for d in g["draws"]} == {True, False}
        assert (g["scales"][:, 0] < 0).any() and (g["scales"][:, 0] > 0).any()
        assert str(g18["augment_rotation"]) == "vertical" and bool(g18["augment_scale_anisotropic"])
        assert g["features"].shape == (lens.sum(), 2) and g["knn"].shape == (lens.sum(), 3) and (g["knn"] >= 0).all()
    assert set(ref.golden_case(Npz(g18), "stop3")["cloud_inds"].tolist()) == {0, 1}


# ------------------------------------------------------------------------------------------------- the ragged k-NN

def test_ragged_restatement_against_a_plain_brute_force():
    rng = np.random.default_rng(4)
    points = (rng.random((300, 3)) * 3).astype(np.float32)
    rows = rng.integers(-2, 302, 120)
    q_off = np.array([0, 40, 40, 110])
    keys = rng.random((3, 70, 3)) * 3
    keys[2, 10] = keys[2, 3]                                            # a duplicate: the lower index first
    valid = rng.random((3, 70)) < 0.6
    valid[2, [3, 10]] = True
    knn, queries = ref.knn_ragged(points, rows, q_off, keys, valid, 4)
    assert (knn[110:] == -1).all() and (queries[110:] == 0).all() and (queries[(rows < 0) | (rows >= 300)] == 0).all()
    for b, (a, e) in enumerate(zip(q_off[:-1], q_off[1:])):
        for s in range(a, e):
            d2 = ((queries[s].astype(np.float64) - keys[b]) ** 2).sum(1)
            cand = sorted((d2[j], j) for j in range(70) if valid[b, j])[:4]
            assert knn[s].tolist() == [j for _, j in cand]
    d3, d10 = ((queries[40:110, None].astype(np.float64) - keys[2][[3, 10]]) ** 2).sum(-1).T
    assert (d3 == d10).all()
    both = (knn[40:110] == 3).any(1) & (knn[40:110] == 10).any(1)
    assert both.any() and all(list(r).index(3) < list(r).index(10) for r in knn[40:110][both])
    assert ref.sanitized_offsets([-3, 7, 5, 99], 20).tolist() == [0, 7, 7, 20]
