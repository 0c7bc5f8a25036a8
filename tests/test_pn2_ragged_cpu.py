"""CPU-only: the ragged point ops' side of the library (exports, header, ABI 9, refusals of the wrappers), the tie-rule
argument of farthest point sampling on a padded block (the key from the padded N orders the points of a smaller cloud
as the key from its own n does), and the host side of predict_whole_scene_grouped(chunks_per_forward=G): chunk_groups and
collate_chunks on CPU tensors."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import chunk_ref
import pn2_ragged_ref
import pn2_ref

RAGGED_EXPORTS = ("mvk_fps_ragged", "mvk_fps_ragged_f64", "mvk_pn2_ball_query_ragged", "mvk_pn2_ball_query_ragged_f64")


def test_library_exports_the_ragged_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in RAGGED_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    # the plain forms' arguments plus one pointer
    for plain, ragged in (("mvk_fps", "mvk_fps_ragged"), ("mvk_pn2_ball_query", "mvk_pn2_ball_query_ragged")):
        for suffix in ("", "_f64"):
            assert len(getattr(lib_mod.lib(), ragged + suffix).argtypes) == \
                len(getattr(lib_mod.lib(), plain + suffix).argtypes) + 1


def test_wrappers_refuse_cpu_tensors_and_malformed_lengths():
    import mvkpconv
    ops = mvkpconv.sub("ops")
    fps_mod = mvkpconv.sub("dropin.mvpnet.ops.fps")
    bq_mod = mvkpconv.sub("dropin.mvpnet.ops.ball_query")
    pts = torch.zeros(2, 8, 3)
    good = torch.tensor([8, 5])
    calls = [lambda l: ops.fps(pts, 2, lengths=l),
             lambda l: ops.pn2_ball_query(pts, pts, 0.1, 4, key_lengths=l),
             lambda l: ops.pn2_ball_query(pts, pts, 0.1, 4, with_distance=True, key_lengths=l),
             lambda l: fps_mod.farthest_point_sample(pts, 2, transpose=False, lengths=l),
             lambda l: bq_mod.ball_query(pts, pts, 0.1, 4, transpose=False, key_lengths=l),
             lambda l: bq_mod.ball_query_distance(pts, pts, 0.1, 4, transpose=False, key_lengths=l)]
    for call in calls:
        with pytest.raises(RuntimeError, match="HBM"):
            call(good)                                                   # a CPU tensor of the right form
        with pytest.raises(RuntimeError, match="int64"):
            call(good.to(torch.int32))
        with pytest.raises(RuntimeError, match="int64"):
            call(good.float())
        with pytest.raises(RuntimeError, match="int64"):
            call([8, 5])
        with pytest.raises(RuntimeError, match="shape"):
            call(torch.tensor([8, 5, 3]))
        with pytest.raises(RuntimeError, match="shape"):
            call(good.view(2, 1))
        with pytest.raises(RuntimeError, match="shape"):
            call(torch.tensor(8))


def test_signatures_gained_trailing_keywords_only():
    import mvkpconv
    ops = mvkpconv.sub("ops")
    tm = mvkpconv.sub("dropin.mvpnet.test_mvpnet_3d")
    wg = mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")
    modules = mvkpconv.sub("dropin.mvpnet.models.pn2.modules")
    names = lambda f: list(inspect.signature(f).parameters)
    assert names(ops.fps) == ["points", "num_centroids", "lengths"]
    assert names(ops.pn2_ball_query) == ["query", "key", "radius", "max_neighbors", "with_distance", "key_lengths"]
    assert names(modules.SetAbstraction.forward) == ["self", "xyz", "feature", "lengths"]
    assert names(modules.QueryGrouper.forward)[-1] == "key_lengths"
    # the grouped loop takes predict_whole_scene's arguments, with its defaults, and the group size behind them
    sig, base = inspect.signature(wg.predict_whole_scene_grouped), inspect.signature(tm.predict_whole_scene)
    assert list(sig.parameters) == list(base.parameters) + ["chunks_per_forward"]
    assert all(sig.parameters[n].default == p.default for n, p in base.parameters.items())
    assert sig.parameters["chunks_per_forward"].default == 1
    for f in (ops.fps, ops.pn2_ball_query, modules.SetAbstraction.forward, modules.QueryGrouper.forward):
        assert inspect.signature(f).parameters[names(f)[-1]].default is None


def test_pn2ssg_refuses_lengths_in_training_and_without_centroids():
    """Both refusals come before any kernel is called, so they show on the host."""
    import mvkpconv
    PN2SSG = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    kw = dict(sa_channels=((8, 8),), radius=(0.3,), max_neighbors=(4,), fp_channels=((8,),), fp_neighbors=(3,),
              seg_channels=(8,), dropout_prob=0.0)
    batch = {"points": torch.zeros(2, 3, 16), "feature": torch.zeros(2, 4, 16), "lengths": torch.tensor([16, 9])}
    net = PN2SSG(4, 3, num_centroids=(8,), **kw)
    with pytest.raises(RuntimeError, match="inference"):
        net.train()(batch)
    for m in (0, -1):
        with pytest.raises(ValueError, match="num_centroids"):
            PN2SSG(4, 3, num_centroids=(m,), **kw).eval()(batch)


# ------------------------------------------------------------------------------------------------ the tie rule

@pytest.mark.parametrize("n, big, m, seed", pn2_ragged_ref.RULE_CASES)
def test_tie_key_of_the_padded_size_orders_a_smaller_cloud_like_its_own(n, big, m, seed):
    j = np.arange(n)
    own, padded = pn2_ref.tie_key(j, n), pn2_ref.tie_key(j, big)
    assert pn2_ref.ref_block(big) > pn2_ref.ref_block(n) or n >= 512      # the keys themselves differ ...
    assert np.array_equal(np.argsort(own), np.argsort(padded))            # ... their order does not (keys are distinct)
    pts = pn2_ref.lattice_cloud(n, seed)
    want = pn2_ref.fps_closed(pts, m)
    assert np.array_equal(pn2_ragged_ref.fps_rule_from(pts, m, big), want)
    assert np.array_equal(pn2_ref.fps_literal(pts, m), want)
    assert not np.array_equal(want, pn2_ref.fps_argmax(pts, m))          # ties were met, and the rule decided them


def test_every_smaller_size_keeps_its_order_under_every_padded_size():
    """A check of the tie-rule ARGUMENT, not of the product: it uses tests/pn2_ref.py only, so it holds with
    or without the ragged kernels. The kernels rely on it by keeping the padded size's key."""
    # over the block sizes 16 .. 512 and beyond the cap
    for big in (16, 31, 64, 130, 257, 1000, 1024, 1025, 4100):
        jb = pn2_ref.tie_key(np.arange(big), big)
        for n in list(range(1, min(big, 1100) + 1, 7)) + [15, 16, 17, 511, 512, 513, 1023]:
            if n <= big:
                assert np.array_equal(np.argsort(pn2_ref.tie_key(np.arange(n), n)), np.argsort(jb[:n])), (n, big)


def test_helper_slices_and_repeats():
    """A check of the test helper tests/pn2_ragged_ref.py itself (the reference of the GPU tests), not of the product."""
    pts = np.stack([pn2_ref.lattice_cloud(40, 31), pn2_ref.lattice_cloud(40, 32)])
    pts[1, 9:] = np.nan                                                   # never read
    got = pn2_ragged_ref.fps(pts, [40, 9], 12)
    assert np.array_equal(got[0], pn2_ref.fps_closed(pts[0], 12))
    assert np.array_equal(got[1, :9], pn2_ref.fps_closed(pts[1, :9], 9)) and (got[1, 9:] == got[1, 8]).all()
    q = pts[:, :5].copy()
    idx, dist = pn2_ragged_ref.ball_query(q, pts, [40, 9], 1.5, 6)
    assert idx[1].max() < 9 and np.array_equal(idx[0], pn2_ref.ball_query(q[:1], pts[:1], 1.5, 6)[0][0])
    assert not np.isnan(dist).any()


# ------------------------------------------------------------------------------------------------ groups of chunks

def chunk(rng, nc, nv=2, k=3, hw=(2, 3)):
    return {"points": torch.from_numpy(rng.random((3, nc)).astype(np.float32)),
            "chunk_ind": torch.from_numpy(rng.permutation(5000)[:nc].astype(np.int64)),
            "images": torch.from_numpy(rng.random((nv, 3) + hw).astype(np.float32)),
            "image_xyz": torch.from_numpy(rng.random((nv,) + hw + (3,)).astype(np.float32)),
            "knn_indices": torch.from_numpy(rng.integers(1, nv * hw[0] * hw[1], size=(nc, k)).astype(np.int64))}


@pytest.fixture(scope="module")
def tm():
    import mvkpconv
    return mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")


SIZES = [50, 20, 64, 33, 7, 41, 90]           # 20 and 7 are sparse at min_nb_pts = 30
MIN_NB = 30


def check_groups(tm, chunks, g_max, want_groups):
    np.random.seed(77)
    got = list(tm.chunk_groups(iter(chunks), g_max, MIN_NB, "cpu"))
    np.random.seed(77)                                                    # the draws of the one-chunk loop, in its order
    rows = [chunk_ref.pad_choice(c["points"].shape[1], MIN_NB) if c["points"].shape[1] < MIN_NB
            else np.arange(c["points"].shape[1]) for c in chunks]
    assert [len(inds) for _, inds in got] == want_groups
    at = 0
    for batch, inds in got:
        group, group_rows = chunks[at:at + len(inds)], rows[at:at + len(inds)]
        at += len(inds)
        sizes = [len(r) for r in group_rows]
        n_max = max(sizes)
        assert set(batch) == {"points", "images", "image_xyz", "knn_indices", "lengths"}
        assert batch["lengths"].dtype == torch.int64 and batch["lengths"].tolist() == sizes
        assert batch["points"].shape == (len(group), 3, n_max) and batch["points"].dtype == torch.float32
        assert batch["knn_indices"].shape == (len(group), n_max, group[0]["knn_indices"].shape[1])
        assert batch["knn_indices"].dtype == torch.int64
        for g, (c, r, ind) in enumerate(zip(group, group_rows, inds)):
            assert ind is c["chunk_ind"]
            assert torch.equal(batch["points"][g, :, :len(r)], c["points"][:, r])
            assert torch.equal(batch["knn_indices"][g, :len(r)], c["knn_indices"][r])
            assert not batch["points"][g, :, len(r):].any() and not batch["knn_indices"][g, len(r):].any()
            assert torch.equal(batch["images"][g], c["images"]) and torch.equal(batch["image_xyz"][g], c["image_xyz"])
    assert at == len(chunks)


@pytest.mark.parametrize("g_max, want", [(2, [2, 2, 2, 1]), (3, [3, 3, 1]), (7, [7]), (32, [7])])
def test_groups_of_g_with_a_short_last_group_and_the_pad_draws_of_the_loop(tm, g_max, want):
    rng = np.random.default_rng(3)
    check_groups(tm, [chunk(rng, n) for n in SIZES], g_max, want)


def test_a_group_closes_early_where_the_shapes_differ(tm):
    rng = np.random.default_rng(4)
    chunks = [chunk(rng, n) for n in SIZES]
    chunks[2] = chunk(rng, SIZES[2], nv=3)                   # other images and image_xyz: a group of its own
    chunks[5] = chunk(rng, SIZES[5], k=5)                    # other k; chunk 6 has the usual k again
    check_groups(tm, chunks, 4, [2, 1, 2, 1, 1])
    chunks = [chunk(rng, n) for n in SIZES]
    chunks[4] = chunk(rng, SIZES[4], hw=(3, 2))              # same element count, another shape
    check_groups(tm, chunks, 3, [3, 1, 1, 2])


def test_collate_refuses_what_does_not_fit_one_batch(tm):
    rng = np.random.default_rng(5)
    strip = lambda c: {k: v for k, v in c.items() if k != "chunk_ind"}
    a, b = strip(chunk(rng, 12)), strip(chunk(rng, 9, nv=3))
    with pytest.raises(ValueError):
        tm.collate_chunks([a, b])
    with pytest.raises(ValueError):
        tm.collate_chunks([])
    one = tm.collate_chunks([a])
    assert one["lengths"].tolist() == [12] and torch.equal(one["points"][0], a["points"])


def test_predict_whole_scene_refuses_a_group_size_below_one(tm):
    with pytest.raises(ValueError, match="chunks_per_forward"):
        tm.predict_whole_scene_grouped(torch.nn.Identity(), torch.zeros(4, 3), [], num_classes=3, chunks_per_forward=0)
