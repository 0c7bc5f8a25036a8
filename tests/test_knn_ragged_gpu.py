"""GPU: mvk_knn_f64_ragged (csrc/sphere_inputs.hip) -- the exact float64 k-NN of B items whose lengths live on the device --
bit for bit against the NumPy restatement (tests/sphere_inputs_ref.py: a float64 lexsort on (d2, index)) AND against the
library's single-item k-NN (ops.knn_pixels -> mvk_knn_f64) on every item alone. Item lengths around the 64-query
workgroup and the 1 024 boundary mixed in one call, key counts below, at and above the 64-key tile, every k whose kernel
differs; items with k-1 and with no valid key, ties, keys far outside the grid torus, a tail behind the total, rows
outside the points, and a q_off that is no running sum. Indices are integers: they compare equal."""
import numpy as np
import pytest
import torch

import sphere_inputs_ref as ref

pytestmark = pytest.mark.gpu

N_POINTS = 5000
LENGTHS = {1: [63], 3: [1, 64, 65], 5: [1023, 0, 1024, 1025, 3000]}
KMAX = 8


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def problem(B, nk, seed, tail=37):
    """points, rows, q_off, keys, valid of B items in a 3 m room; cap = the total + tail."""
    rng = np.random.default_rng(seed)
    points = (rng.random((N_POINTS, 3)) * 3.0).astype(np.float32)
    lens = LENGTHS[B]
    q_off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, N_POINTS, int(q_off[-1]) + tail).astype(np.int64)
    keys = rng.random((B, nk, 3)) * 3.0
    valid = rng.random((B, nk)) < 0.7
    valid[:, :min(nk, 2)] = True
    return points, rows, q_off, keys, valid


_REFERENCE = {}


def reference(B, nk):
    """The problem and its KMAX nearest neighbours, computed once: the k nearest are the first k columns."""
    if (B, nk) not in _REFERENCE:
        p = problem(B, nk, 100 * B + nk)
        _REFERENCE[(B, nk)] = (p, ref.knn_ragged(*p, KMAX))
    return _REFERENCE[(B, nk)]


def run(ops, points, rows, q_off, keys, valid, k, **kw):
    return ops.knn_f64_ragged(dev(points), dev(rows), dev(q_off), dev(keys), None if valid is None else dev(valid), k=k, **kw)


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("nk", [2, 64, 65, 4100])
@pytest.mark.parametrize("B", [1, 3, 5])
def test_ragged_equals_the_restatement_and_the_single_item_knn(ops, B, nk, k):
    (points, rows, q_off, keys, valid), (knn8, queries) = reference(B, nk)
    got, got_q = run(ops, points, rows, q_off, keys, valid, k, return_queries=True)
    got, got_q = got.cpu().numpy(), got_q.cpu().numpy()
    want = knn8[:, :k]                                 # an item with fewer valid keys already holds its -1 there
    assert got.dtype == np.int64 and got.shape == want.shape
    assert np.array_equal(got_q.view(np.uint32), queries.view(np.uint32))
    assert np.array_equal(got, want)
    assert (got[q_off[-1]:] == -1).all() and (got_q[q_off[-1]:] == 0).all()          # the tail behind the total
    for b in range(B):                                                               # mvk_knn_f64 on the item alone
        a, e = q_off[b], q_off[b + 1]
        if e > a:
            alone = ops.knn_pixels(dev(queries[a:e]), dev(keys[b]), dev(valid[b]), k=k).cpu().numpy()
            assert np.array_equal(got[a:e], alone), "item %d" % b


def test_items_with_too_few_and_with_no_valid_key(ops):
    (points, rows, q_off, keys, valid), _ = reference(3, 65)
    valid = valid.copy()
    valid[0] = False
    valid[0, [7, 40]] = True                           # k - 1 valid keys
    valid[1] = False                                   # none
    want, _ = ref.knn_ragged(points, rows, q_off, keys, valid, 3)
    got = run(ops, points, rows, q_off, keys, valid, 3).cpu().numpy()
    assert np.array_equal(got, want)
    assert (got[q_off[0]:q_off[1], 2] == -1).all() and (got[q_off[0]:q_off[1], :2] >= 0).all()
    assert (got[q_off[1]:q_off[2]] == -1).all() and (got[q_off[2]:q_off[3]] >= 0).all()


def test_ties_go_to_the_lower_index(ops):
    """Every key occurs twice and every second query lies on a key: equal distances inside the first k + 1."""
    (points, rows, q_off, keys, valid), _ = reference(5, 65)
    keys, points = keys.copy(), points.copy()
    keys[:, 1::2] = keys[:, 0:-1:2]
    valid = np.ones_like(valid)
    on = keys[0, ::2].astype(np.float32)               # queries that coincide with (the float32 rounding of) keys
    keys[:, :64:2] = on[:32].astype(np.float64)
    keys[:, 1:64:2] = on[:32].astype(np.float64)
    points[:32] = on[:32]
    rows = rows.copy()
    rows[::2] = np.arange(len(rows[::2])) % 32
    want, queries = ref.knn_ragged(points, rows, q_off, keys, valid, 3)
    a, e = q_off[4], q_off[5]
    d = queries[a:e, None, :].astype(np.float64) - keys[4][want[a:e]]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    tied = d2[:, 0] == d2[:, 1]
    assert tied.any() and (want[a:e][tied, 0] < want[a:e][tied, 1]).all()             # a tie is present, lower index first
    assert (d2[::2, 0] == 0).all()
    got = run(ops, points, rows, q_off, keys, valid, 3).cpu().numpy()
    assert np.array_equal(got, want)


def test_keys_far_outside_the_grid_torus(ops):
    """The 32^3 grid of 0.1 m cells wraps every 3.2 m: binning decides the order of the visit only."""
    (points, rows, q_off, keys, valid), _ = reference(5, 4100)
    keys = keys.copy()
    keys[0] += 1000.0
    keys[1, ::3] += np.array([3.2, -6.4, 32.0])        # the same cells, far apart
    keys[2, ::5] *= 1.0e6
    keys[3] -= 77.7
    want, _ = ref.knn_ragged(points, rows, q_off, keys, valid, 3)
    got = run(ops, points, rows, q_off, keys, valid, 3).cpu().numpy()
    assert np.array_equal(got, want)


def test_rows_outside_the_points_give_a_zero_query(ops):
    (points, rows, q_off, keys, valid), _ = reference(3, 64)
    rows = rows.copy()
    rows[[0, 5, 70]] = [-1, N_POINTS, 1 << 40]
    want, queries = ref.knn_ragged(points, rows, q_off, keys, valid, 3)
    assert (queries[[0, 5, 70]] == 0).all()
    got, got_q = run(ops, points, rows, q_off, keys, valid, 3, return_queries=True)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_q.cpu().numpy(), queries)


def test_offsets_that_are_no_running_sum_stay_inside_the_buffers(ops):
    """q_off is read clamped to [0, cap] and as its running maximum: the result is defined."""
    (points, rows, _, keys, valid), _ = reference(3, 64)
    cap = rows.shape[0]
    q_off = np.array([-5, 50, 20, 1 << 40], np.int64)  # -> 0, 50, 50, cap
    assert ref.sanitized_offsets(q_off, cap).tolist() == [0, 50, 50, cap]
    want, queries = ref.knn_ragged(points, rows, q_off, keys, valid, 3)
    got, got_q = run(ops, points, rows, q_off, keys, valid, 3, return_queries=True)
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(got_q.cpu().numpy(), queries)
    assert (want >= 0).all()


def test_sizes_are_checked_before_the_call(ops):
    (points, rows, q_off, keys, valid), _ = reference(1, 2)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.knn_f64_ragged(torch.from_numpy(points), dev(rows), dev(q_off), dev(keys))
    with pytest.raises(RuntimeError, match="k=9"):
        run(ops, points, rows, q_off, keys, valid, 9)
    with pytest.raises(RuntimeError, match="q_off"):
        run(ops, points, rows, q_off[:1], keys, valid, 3)
    with pytest.raises(RuntimeError, match="keys"):
        ops.knn_f64_ragged(dev(points), dev(rows), dev(q_off), dev(keys.astype(np.float32)))
