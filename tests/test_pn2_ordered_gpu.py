"""GPU: the ordered forms of the two scattering PointNet++ backwards (csrc/pn2_ordered.hip) -- the transposed index as a
CSR and the per-key gathers behind ops.set_deterministic(True) -- against the NumPy oracle tests/pn2_ordered_ref.py:
exact equality for the CSR, bit equality for the gradients in float32 and float64."""
import contextlib

import numpy as np
import pytest
import torch

import pn2_ordered_ref as ref
import pn2_ref
import util
from test_pn2_gpu import NET_KW, U, interp_case

pytestmark = pytest.mark.gpu

DTYPES = [np.float32, np.float64]
WAVE_ROW = 512                                    # csrc/pn2_ordered.hip CSR_WAVE_ROW: longer rows take the rescan path


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module")
def g16(golden):
    return golden("g16_pn2ssg")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


@contextlib.contextmanager
def deterministic(ops):
    was = ops.is_deterministic()
    ops.set_deterministic(True)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ the CSR

def one_key(b, n2, k, n1, key):
    return np.full((b, n2, k), key, np.int64)


def two_long_rows():
    """Keys 1 and 2 of five own 3 072 positions each, interleaved: two rescans in one workgroup of four rows."""
    index = np.empty((1, 192, 32), np.int64)
    index.reshape(-1)[0::2] = 1
    index.reshape(-1)[1::2] = 2
    return index


def at_the_threshold():
    """Rows of exactly WAVE_ROW and WAVE_ROW + 1 entries (the last a wave ranks, the first that is rescanned), a short
    one between them, shuffled; the second batch element keeps every row short."""
    rng = np.random.default_rng(12)
    keys = np.concatenate([np.full(WAVE_ROW, 0), np.full(WAVE_ROW + 1, 2), np.full(7, 1), np.full(4, 5)])
    index = np.stack([rng.permutation(keys), rng.integers(0, 6, keys.size)])
    return index.astype(np.int64)[:, :, None]                         # (2, 1036, 1): K = 1 as well


CSR_CASES = {
    "random K=3": lambda: (np.random.default_rng(1).integers(0, 129, (3, 513, 3)), 129),
    "random K=33": lambda: (np.random.default_rng(2).integers(0, 513, (5, 129, 33)), 513),
    "one key L=1536": lambda: (one_key(2, 512, 3, 64, 32), 64),
    "one key L=6144": lambda: (one_key(1, 192, 32, 5, 3), 5),
    "two long rows": lambda: (two_long_rows(), 5),
    "threshold": lambda: (at_the_threshold(), 6),
    "ball query like": lambda: (ref.ball_like_index(3, 129, 16, 200, seed=7), 200),
    "K=1": lambda: (np.random.default_rng(3).integers(0, 9, (2, 70, 1)), 9),
    "N1=1": lambda: (np.zeros((2, 70, 3), np.int64), 1),
    "B=1": lambda: (np.random.default_rng(4).integers(0, 300, (1, 65, 4)), 300),
    "N2=0": lambda: (np.zeros((2, 0, 3), np.int64), 17),
    "flat (B, L)": lambda: (np.random.default_rng(5).integers(-1, 40, (2, 777)), 37),
}


@pytest.mark.parametrize("name", list(CSR_CASES))
def test_index_csr_equals_the_oracle(ops, name):
    index, n1 = CSR_CASES[name]()
    index = index.astype(np.int64)
    want_rows, want_entries = ref.csr(index, n1)
    out_of_range = bool(((index < 0) | (index >= n1)).any())
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    for word in (status, None):
        row_start, entries = ops.index_csr(dev(index), n1, word)
        assert row_start.dtype == torch.int32 and entries.dtype == torch.int32
        assert tuple(row_start.shape) == (index.shape[0] * n1 + 1,) and entries.numel() == index.size
        assert np.array_equal(host(row_start), want_rows), name
        assert np.array_equal(host(entries)[:want_entries.size], want_entries), name
    assert int(status.item()) == int(out_of_range)      # set exactly when an entry is out of range (and a word was passed)


def test_index_csr_status_word_is_only_ever_raised(ops):
    status = torch.zeros(1, dtype=torch.int32, device="cuda")
    good = dev(np.random.default_rng(6).integers(0, 8, (2, 33, 3)))
    bad = good.clone()
    bad[1, 20, 2] = 8
    ops.index_csr(good, 8, status)
    assert int(status.item()) == 0
    ops.index_csr(bad, 8, None)
    assert int(status.item()) == 0
    ops.index_csr(bad, 8, status)
    ops.index_csr(good, 8, status)                     # a later clean build does not clear it
    assert int(status.item()) == 1


# ------------------------------------------------------------------------------------------------ the two backwards

def run_twice(fn):
    first, second = fn(), fn()
    assert same_bits(first, second)                    # the same sums in the same order
    return first


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("b, c, n1, n2, same_index", [(2, 64, 128, 512, False), (3, 65, 129, 513, False),
                                                      (2, 5, 64, 512, True)])
def test_interpolation_backward_is_the_ordered_sum(ops, b, c, n1, n2, same_index, dtype):
    f, idx, w, go = interp_case(b, c, n1, n2, same_index)
    f, w, go = f.astype(dtype), w.astype(dtype), go.astype(dtype)
    want = ref.interpolate_bwd(go, idx, w, n1)

    def backward():
        ft = dev(f).requires_grad_(True)
        ops.feature_interpolate(ft, dev(idx), dev(w)).backward(dev(go))
        return host(ft.grad)

    with deterministic(ops):
        got = run_twice(backward)
    assert got.dtype == dtype and same_bits(got, want)
    count = ref.counts(idx, n1)
    empty = np.broadcast_to(count[:, None, :] == 0, got.shape)
    assert same_bits(got[empty], np.zeros(int(empty.sum()), dtype))    # +0, not merely == 0
    if same_index:
        assert empty.any() and count.max() == 3 * n2                   # one row of 1 536 entries, the others empty
    # inside the rounding bound of the atomic path's test (any order of the same rounded products)
    wide = np.float64 if dtype == np.float32 else np.longdouble
    exact, scale, cnt = pn2_ref.interpolate_bwd(go, idx, w, n1, wide)
    assert np.array_equal(cnt, count)
    assert np.all(np.abs(got.astype(wide) - exact) <= (cnt[:, None, :] + 1) * U[dtype] * scale)
    ops.pn2_check_indices()


def group_case(name):
    if name == "padded":
        b, c, n1, n2, k = 3, 7, 400, 129, 16
        index = ref.ball_like_index(b, n2, k, n1, seed=7)
    else:
        b, c, n1, n2, k = name
        keys = np.arange(n1)
        index = np.random.default_rng(n1).choice(keys[keys % 7 != 3], (b, n2, k))      # every seventh key has no entry
    grad_out = np.random.default_rng(k).standard_normal((b, c, n2, k))
    return index.astype(np.int64), grad_out, n1


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", [(2, 3, 512, 128, 32), (5, 64, 513, 129, 33), "padded"])
def test_group_points_backward_is_the_ordered_sum(ops, case, dtype):
    index, go, n1 = group_case(case)
    go = go.astype(dtype)
    b, c = go.shape[:2]
    want = ref.group_points_bwd(go, index, n1)

    def backward():
        pts = torch.zeros((b, c, n1), dtype=torch.float64 if dtype == np.float64 else torch.float32,
                          device="cuda").requires_grad_(True)
        ops.group_points(pts, dev(index)).backward(dev(go))
        return host(pts.grad)

    with deterministic(ops):
        got = run_twice(backward)
    assert got.dtype == dtype and same_bits(got, want)
    empty = np.broadcast_to(ref.counts(index, n1)[:, None, :] == 0, got.shape)
    assert empty.any() and same_bits(got[empty], np.zeros(int(empty.sum()), dtype))
    # the existing rounding bound, written for this op: T terms added in T roundings, any order
    wide = np.float64 if dtype == np.float32 else np.longdouble
    flat, ix = go.reshape(b, c, -1).astype(wide), ref.flat_index(index)
    exact, scale = ref._ordered(flat, ix, n1), ref._ordered(np.abs(flat), ix, n1)
    cnt = ref.counts(index, n1)
    assert np.all(np.abs(got.astype(wide) - exact) <= (cnt[:, None, :] + 1) * U[dtype] * scale)


def test_default_mode_keeps_the_atomic_backward_and_builds_nothing(ops):
    assert not ops.is_deterministic()
    index, go, n1 = group_case((2, 3, 512, 128, 32))
    idx = dev(index)
    pts = torch.zeros((2, 3, n1), device="cuda").requires_grad_(True)
    ops.group_points(pts, idx).backward(dev(go.astype(np.float32)))
    assert ops.index_csr_for(idx, n1) is None
    with deterministic(ops):                            # nor when no gradient is asked for
        with torch.no_grad():
            ops.group_points(pts, idx)
        ops.group_points(pts.detach(), idx)
        assert ops.index_csr_for(idx, n1) is None


def test_one_index_serves_both_uses_of_a_grouper(ops):
    b, n1, n2, k = 2, 300, 65, 16
    index = ref.ball_like_index(b, n2, k, n1, seed=21)
    idx, other = dev(index), dev(index)                 # the same values in another tensor object
    rng = np.random.default_rng(22)
    g_xyz = rng.standard_normal((b, 3, n2, k)).astype(np.float32)
    g_feat = rng.standard_normal((b, 20, n2, k)).astype(np.float32)
    xyz = torch.randn(b, 3, n1, device="cuda").requires_grad_(True)
    feat = torch.randn(b, 20, n1, device="cuda").requires_grad_(True)
    built = []
    real = ops.index_csr

    def counting(*args, **kwargs):
        built.append(1)
        return real(*args, **kwargs)

    with deterministic(ops):
        ops.index_csr = counting
        try:
            loss = (ops.group_points(xyz, idx) * dev(g_xyz)).sum() + (ops.group_points(feat, idx) * dev(g_feat)).sum()
            assert ops.index_csr_for(idx, n1) is None   # nothing is built before a gradient is asked for
            loss.backward()
        finally:
            ops.index_csr = real
        assert len(built) == 1
        csr = ops.index_csr_for(idx, n1)
        assert csr is not None and ops.index_csr_for(idx, n1) is csr
        assert ops.index_csr_for(other, n1) is None and ops.index_csr_for(idx, n1 + 1) is None
        assert same_bits(host(xyz.grad), ref.group_points_bwd(g_xyz, index, n1))
        assert same_bits(host(feat.grad), ref.group_points_bwd(g_feat, index, n1))
        want_rows, want_entries = ref.csr(index, n1)
        assert np.array_equal(host(csr[0]), want_rows) and np.array_equal(host(csr[1])[:want_entries.size], want_entries)
        # a second graph over the same index finds the same object; the other tensor gets a CSR of its own
        xyz.grad = None
        ops.group_points(xyz, idx).backward(dev(g_xyz))
        assert ops.index_csr_for(idx, n1) is csr
        ops.group_points(xyz, other).backward(dev(g_xyz))
        assert ops.index_csr_for(other, n1) is not None and ops.index_csr_for(other, n1) is not csr
        # written in place, the index no longer matches what was built for it
        idx[0, 0, 0] = 5
        assert ops.index_csr_for(idx, n1) is None


def test_out_of_range_index_in_deterministic_mode_is_an_error_not_a_fault(ops):
    f = dev(np.ones((1, 2, 8), np.float32)).requires_grad_(True)
    w = dev(np.full((1, 4, 3), 1 / 3, np.float32))
    with deterministic(ops):
        ops.pn2_check_indices()                             # start from a clear status word
        for bad in (8, -1):
            idx = np.zeros((1, 4, 3), np.int64)
            idx[0, 2, 1] = bad
            out = ops.feature_interpolate(f, dev(idx), w)
            with pytest.raises(RuntimeError, match="outside"):
                ops.pn2_check_indices()
            out.sum().backward()                            # the entry is in no row: it contributes nothing
            assert np.allclose(host(f.grad)[0, :, 0], 11 / 3) and np.all(host(f.grad)[0, :, 1:] == 0)
            f.grad = None
            with pytest.raises(RuntimeError, match="outside"):
                ops.pn2_check_indices()                     # and the CSR build of the backward reported it
            ops.pn2_check_indices()


def test_csr_build_and_backward_replay_from_a_graph(ops):
    b, c, n1, n2 = 2, 9, 70, 300
    rng = np.random.default_rng(31)
    idx = rng.integers(0, n1, (b, n2, 3))
    w = rng.random((b, n2, 3)).astype(np.float32)
    grads = [rng.standard_normal((b, c, n2)).astype(np.float32) for _ in range(3)]
    with deterministic(ops):
        ops.pn2_check_indices()                             # the status word exists before the capture
        f = torch.zeros((b, c, n1), device="cuda").requires_grad_(True)
        d_idx, d_w, go = dev(idx), dev(w), dev(grads[0])
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):                       # one eager pass on the capture's stream first
            (warm,) = torch.autograd.grad(ops.feature_interpolate(f, d_idx, d_w), f, go)
        torch.cuda.current_stream().wait_stream(side)
        assert same_bits(host(warm), ref.interpolate_bwd(grads[0], idx, w, n1))
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            (gi,) = torch.autograd.grad(ops.feature_interpolate(f, d_idx, d_w), f, go)
        for g in grads[1:]:
            go.copy_(dev(g))
            graph.replay()
            assert same_bits(host(gi), ref.interpolate_bwd(g, idx, w, n1))
        ops.pn2_check_indices()


# ------------------------------------------------------------------------------------------------ the network

def test_pn2ssg_gradients_in_deterministic_mode(ops, g16):
    import mvkpconv
    PN2SSG = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    net = PN2SSG(**NET_KW).cuda()
    net.load_state_dict({k[3:]: torch.from_numpy(v) for k, v in g16.items() if k.startswith("sd/")}, strict=True)
    batch = {"points": dev(g16["points"]), "feature": dev(g16["feature"])}
    failures = []
    net.train()
    with deterministic(ops):
        out = net(batch)["seg_logit"]
        util.referee_check("g16 PN2SSG train logits", host(out.detach()), g16["logit_train_f32"], g16["logit_train_f64"],
                           failures=failures)
        out.square().mean().backward()
        torch.cuda.synchronize()
    names = [n for n, _ in net.named_parameters()]
    assert sorted(names) == sorted(k[len("grad_f64/"):] for k in g16 if k.startswith("grad_f64/"))
    for name, p in net.named_parameters():
        util.referee_check("g16 PN2SSG grad " + name, host(p.grad), g16["grad_f32/" + name], g16["grad_f64/" + name],
                           failures=failures)
    assert not failures, "\n".join(failures)
    ops.pn2_check_indices()
