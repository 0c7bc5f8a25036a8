"""GPU parity tests proper: the HIP path (through the C ABI) against (a) golden vectors captured from
the reference and (b) the CPU oracle on seeded inputs. Bit-exact for index / subsampling work,
1e-4 relative (north_star) for KPConv floating point."""
import importlib
import os

import numpy as np
import pytest
import torch

from conftest import load_golden
from util import bits_equal, assert_neighbors_equal_mod_ties, rel_err, check_err

pytestmark = pytest.mark.gpu

PKG = "enhancing-3d-point-cloud-segmentation-using-multi-modal-fusion-with-2d-images_amd"
FP_TOL = 1e-4   # north_star: "within 1e-4 rel for KPConv float outputs"
DEFORM_TOL = 1e-4   # gradients through the offset branch of the deformable operator: the north_star bar (measured <= 5.2e-7, profiles/r03_parity_errors.txt; was 5e-4)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return importlib.import_module(PKG + ".ops")


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ------------------------------------------------------------------ subsampling

@pytest.mark.parametrize("name", ["g1_sub_4096", "g1_sub_batch", "g1_sub_maxp"])
def test_subsample_golden_bit_exact(ops, name):
    g = load_golden(name)
    sp, sl = ops.grid_subsample_batch(T(g["points"]), g["lens"], dl=float(g["dl"]), max_p=int(g.get("max_p", 0)))
    assert np.array_equal(sl, g["out_lens"])
    assert bits_equal(sp.cpu().numpy(), g["out_points"])


def test_subsample_features_labels_golden(ops):
    g = load_golden("g1_sub_feat_lab")
    n = g["points"].shape[0]
    sp, sl, sf, slab = ops.grid_subsample_batch(T(g["points"]), [n], features=T(g["features"]),
                                                labels=T(g["labels"]), dl=float(g["dl"]))
    assert bits_equal(sp.cpu().numpy(), g["out_points"]) and bits_equal(sf.cpu().numpy(), g["out_features"])
    assert np.array_equal(slab.cpu().numpy(), g["out_labels"])      # incl. tie-broken majority votes


def test_subsample_labels_vs_oracle_many_classes(ops):
    from oracle import cport
    rng = np.random.default_rng(11)
    p = (rng.random((20000, 3)) * [2, 2, 1]).astype(np.float32)
    lab = rng.integers(-5, 45, (20000, 2)).astype(np.int32)           # > 13 distinct labels per voxel: rehash epochs
    want = cport.subsample_batch(p, [20000], labels=lab, dl=0.5)
    got = ops.grid_subsample_batch(T(p), [20000], labels=T(lab), dl=0.5)
    assert bits_equal(got[0].cpu().numpy(), want[0]) and np.array_equal(got[2].cpu().numpy(), want[2])


@pytest.mark.parametrize("n,dl,seed", [(1, 0.1, 0), (13, 0.5, 1), (14, 0.01, 2), (777, 0.05, 3),
                                        (20000, 0.04, 4), (200000, 0.03, 5)])
def test_subsample_vs_oracle(ops, n, dl, seed):
    # (13, ...) and (14, ...) count POINTS, not voxels: uniform clouds do not pin the unordered_map's rehash thresholds.
    # Voxel counts at 13, 29, 59, ... +-1, voxel-edge, same-bucket and duplicate clouds: test_cloud_cases_gpu.py.
    from oracle import cport
    rng = np.random.default_rng(seed)
    p = (rng.random((n, 3)) * [3, 2, 1]).astype(np.float32)
    lens = np.array([n // 3, 0, n - n // 3], np.int32) if n > 20 else np.array([n], np.int32)
    want = cport.subsample_batch(p, lens, dl=dl)
    got = ops.grid_subsample_batch(T(p), lens, dl=dl)
    assert np.array_equal(got[1], want[1])
    assert bits_equal(got[0].cpu().numpy(), want[0])


def test_subsample_idempotent_full_size(ops):
    """Size-independent property at BASELINE size: subsampling barycentres again at the same dl with
    an unrotated grid keeps the count within the voxel bound and every output inside its voxel."""
    rng = np.random.default_rng(9)
    p = (rng.random((400000, 3)) * [2.4, 2.4, 2.4]).astype(np.float32)
    sp, sl = ops.grid_subsample_batch(T(p), [p.shape[0]], dl=0.04)
    assert sl[0] == sp.shape[0] <= 61 ** 3
    sp2, sl2 = ops.grid_subsample_batch(sp, sl, dl=0.04)
    assert sl2[0] <= sl[0]


# ------------------------------------------------------------------ neighbours

def test_neighbors_conv_golden_exact(ops):
    g = load_golden("g2_nb_conv_b1")
    nb = ops.radius_neighbors_batch(T(g["queries"]), T(g["supports"]), g["q_lens"], g["s_lens"], float(g["radius"]))
    assert nb.dtype == torch.int32 and np.array_equal(nb.cpu().numpy(), g["out"])


def test_neighbors_volumetric_golden_exact(ops):
    g = load_golden("g2_nb_volumetric")
    nb = ops.radius_neighbors_batch(T(g["queries"]), T(g["supports"]), g["q_lens"], g["s_lens"], float(g["radius"]))
    assert np.array_equal(nb.cpu().numpy(), g["out"])


def test_neighbors_ragged_golden_mod_ties_and_oracle_exact(ops):
    from oracle import cport
    g = load_golden("g2_nb_pool_up_b3")
    c, f, cl, fl = g["coarse"], g["fine"], g["coarse_lens"], g["fine_lens"]
    pool = ops.radius_neighbors_batch(T(c), T(f), cl, fl, float(g["r_pool"])).cpu().numpy()
    up = ops.radius_neighbors_batch(T(f), T(c), fl, cl, float(g["r_up"])).cpu().numpy()
    assert_neighbors_equal_mod_ties(pool, g["out_pool"], c, f, cl, fl)
    assert_neighbors_equal_mod_ties(up, g["out_up"], f, c, fl, cl)
    # against the oracle the order is exact (same (d2, index) rule)
    assert np.array_equal(pool, cport.radius_neighbors_batch(c, f, cl, fl, float(g["r_pool"])))
    assert np.array_equal(up, cport.radius_neighbors_batch(f, c, fl, cl, float(g["r_up"])))
    # limit = crop to the nearest columns
    lim = ops.radius_neighbors_batch(T(c), T(f), cl, fl, float(g["r_pool"]), limit=7).cpu().numpy()
    assert np.array_equal(lim, pool[:, :7])


def test_neighbors_vs_oracle_seeded(ops):
    from oracle import cport
    rng = np.random.default_rng(3)
    s = (rng.random((6000, 3)) * [1.5, 1.5, 0.2]).astype(np.float32)
    q = (rng.random((2500, 3)) * [1.8, 1.5, 0.3] - 0.1).astype(np.float32)   # some queries outside the grid
    ql, sl = np.array([1000, 0, 1500], np.int32), np.array([2500, 500, 3000], np.int32)
    for r in (0.03, 0.11, 0.4):
        want = cport.radius_neighbors_batch(q, s, ql, sl, r)
        got = ops.radius_neighbors_batch(T(q), T(s), ql, sl, r).cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want)


def test_neighbors_properties_full_size(ops):
    """BASELINE-size (20k-point level-0 cloud) properties: sorted rows, self first, symmetric membership."""
    rng = np.random.default_rng(5)
    raw = (rng.random((300000, 3)) * [2.4, 2.4, 0.05]).astype(np.float32)
    p, l = ops.grid_subsample_batch(T(raw), [raw.shape[0]], dl=0.04)
    nb = ops.radius_neighbors_batch(p, p, l, l, 0.1)
    N = p.shape[0]
    assert (nb[:, 0].cpu() == torch.arange(N, dtype=torch.int32)).all()      # d2 = 0 first
    pp = torch.cat([p, torch.full((1, 3), 1e6, device="cuda")])
    d2 = ((pp[nb.long()] - p[:, None, :]) ** 2).sum(-1)
    d2 = torch.where(nb == N, torch.full_like(d2, 3e38), d2)
    assert (d2[:, 1:] >= d2[:, :-1]).all()
    counts = (nb < N).sum(1)
    back = torch.zeros(N, dtype=torch.int64, device="cuda").index_add_(
        0, nb[nb < N].long(), torch.ones(int(counts.sum()), dtype=torch.int64, device="cuda"))
    assert (back == counts).all()                                             # symmetric relation


def test_neighbors_enqueue_only_and_grid_reuse_equal_the_synchronous_search(ops):
    """mvk_radius_neighbors_enqueue (no read-back, shared cell grid) fills exactly the rows the classic
    call fills; the status word carries the max row count; the pyramid built that way equals the
    synchronous pyramid column for column."""
    rng = np.random.default_rng(11)
    raw = (rng.random((120000, 3)) * [2.0, 2.0, 0.6]).astype(np.float32)
    lens0 = [70000, 50000]
    p, l = ops.grid_subsample_batch(T(raw), lens0, dl=0.04)
    sub, ls = ops.grid_subsample_batch(p, l, dl=0.08)
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    ref_conv = ops.radius_neighbors_batch(p, p, l, l, 0.1, limit=30)
    ref_pool = ops.radius_neighbors_batch(sub, p, ls, l, 0.1, limit=30)
    conv = ops.radius_neighbors_batch(p, p, l, l, 0.1, limit=30, status=status)                       # builds the grid
    pool = ops.radius_neighbors_batch(sub, p, ls, l, 0.1, limit=30, status=status, reuse_grid=True)   # reuses it
    assert conv.shape[1] == 30 and torch.equal(conv[:, :ref_conv.shape[1]], ref_conv)
    assert torch.equal(pool[:, :ref_pool.shape[1]], ref_pool)
    assert (conv[:, ref_conv.shape[1]:] == p.shape[0]).all() and (pool[:, ref_pool.shape[1]:] == p.shape[0]).all()
    full = ops.radius_neighbors_batch(p, p, l, l, 0.1)
    assert ops.check_neighbor_status(status) == full.shape[1]

    import importlib
    common = importlib.import_module(PKG + ".dropin.datasets.common")
    syn = importlib.import_module(PKG + ".synthetic")
    cfg = syn.make_config("baseline")
    rots = [np.stack([np.eye(3, dtype=np.float32)] * 2) for _ in range(4)]
    limits = [30, 28, 30, 32, 20]
    a = common.segmentation_inputs_sphere(cfg, p, np.asarray(l), limits, torch.int32, rots)
    status.zero_()
    b = common.segmentation_inputs_sphere(cfg, p, np.asarray(l), limits, torch.int32, rots, status=status)
    ops.check_neighbor_status(status)
    for key in ("neighbors", "pools", "upsamples"):
        for x, y in zip(a[key], b[key]):
            if x.numel() == 0:
                continue
            assert torch.equal(y[:, :x.shape[1]], x), key
    for x, y in zip(a["points"], b["points"]):
        assert torch.equal(x, y)


def test_device_lens_variants_edge_cases(ops):
    """mvk_grid_subsample_batch_dev / mvk_radius_neighbors_dev: an empty cloud inside the batch, rows past
    the device-side counts, and an output capacity that is too small (flagged, nothing written past it)."""
    rng = np.random.default_rng(21)
    a = (rng.random((30000, 3)) * [1.5, 1.5, 0.3]).astype(np.float32)
    b = (rng.random((20000, 3)) * [1.0, 1.0, 0.3] + 5).astype(np.float32)
    lens_h = [30000, 0, 20000]
    pts = T(np.concatenate([a, b, np.full((777, 3), 1e6, np.float32)]))          # 777 padding rows
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    want_p, want_l = ops.grid_subsample_batch(pts[:50000], lens_h, dl=0.06)
    M = want_p.shape[0]
    status = torch.zeros(2, dtype=torch.int32, device="cuda")
    out = torch.full((M + 100, 3), -1.0, device="cuda")
    out_l = torch.zeros(3, dtype=torch.int32, device="cuda")
    tot = torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.grid_subsample_dev(pts, lens, 0.06, out, out_l, status, total_out=tot)
    assert torch.equal(out[:M], want_p) and (out[M:] == 1e6).all()
    assert out_l.cpu().tolist() == list(want_l) and int(tot) == M and int(status[1]) == 0
    # neighbours: queries = subsampled clouds (capacity M + 100), supports = input clouds (capacity 50 777)
    ref = ops.radius_neighbors_batch(want_p, pts[:50000], want_l, lens_h, 0.08, limit=40)
    nb = torch.full((M + 100, 40), -7, dtype=torch.int32, device="cuda")
    ops.radius_neighbors_dev(out, pts, out_l, lens, 0.08, nb, 123456, status)
    w = ref.shape[1]
    body = nb[:M, :w]
    assert torch.equal(torch.where(body == 123456, torch.full_like(body, 50000), body), ref)
    assert (nb[:M, w:] == 123456).all() and (nb[M:] == 123456).all()
    assert 40 < ops.check_neighbor_status(status) <= 256
    # a row with more in-range supports than the 256-entry list of the narrow searches: flagged, loudly
    dense = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.radius_neighbors_dev(out, pts, out_l, lens, 0.3, nb, 123456, dense)
    with pytest.raises(RuntimeError):
        ops.check_neighbor_status(dense)
    # capacity too small: flagged, rows beyond the capacity are dropped, the guard row stays untouched
    small = torch.full((M - 50 + 1, 3), -1.0, device="cuda")
    ops.grid_subsample_dev(pts, lens, 0.06, small[:M - 50], out_l, status, total_out=tot)
    assert int(status[1]) == 1 and (small[M - 50] == -1).all() and torch.equal(small[:M - 50], want_p[:M - 50])
    with pytest.raises(RuntimeError):
        ops.check_neighbor_status(status)


def test_neighbor_workspace_shared_by_searches_of_different_query_counts(ops):
    """The three users of the neighbour workspace layout on ONE workspace with different query capacities: a search,
    a search with fewer queries that reuses its grid, and the cell-order work list -- the grid part of the layout
    must not move with the query count."""
    rng = np.random.default_rng(31)
    cloud = rng.random((400, 3)).astype(np.float32)
    lens_h = [200, 0, 200]                                               # an empty cloud in the middle
    pts = T(np.concatenate([cloud, np.full((200, 3), 1e6, np.float32)]))           # capacity 600
    lens = torch.tensor(lens_h, dtype=torch.int32, device="cuda")
    q_lens = torch.tensor([200, 0, 56], dtype=torch.int32, device="cuda")         # the first 256 capacity rows
    status = torch.zeros(2, dtype=torch.int32, device="cuda")

    def search(nq, ql, reuse, **rev):
        out = torch.full((nq, 64), -7, dtype=torch.int32, device="cuda")
        ops.radius_neighbors_dev(pts[:nq], pts, ql, lens, 0.15, out, 600, status, reuse_grid=reuse, **rev)
        return out

    full = search(600, lens, False)                                             # (a)
    order_a = ops.neighbors_cell_order(600, 600, 3, s_lens_dev=lens)
    reused = search(256, q_lens, True)                                          # (b): the grid of (a)
    order_c = ops.neighbors_cell_order(256, 600, 3, s_lens_dev=lens)            # (c)
    fresh = search(256, q_lens, False)
    assert torch.equal(reused, fresh) and torch.equal(reused, full[:256])
    assert torch.equal(order_c, order_a)
    assert sorted(order_a[:400].cpu().tolist()) == list(range(400)) and order_a[400:].cpu().tolist() == list(range(400, 600))
    longest, overflow = status.cpu().tolist()
    assert overflow == 0 and 1 <= longest <= 64, (longest, overflow)            # about 3 supports in range of a query
    assert (full[400:] == 600).all() and (full[:400, 0] == torch.arange(400, device="cuda")).all()
    # once more with the search filling the transposed relation itself
    rev = torch.full((600, 64), -7, dtype=torch.int32, device="cuda")
    counts = torch.zeros(600, dtype=torch.int32, device="cuda")
    rev_status = torch.zeros(2, dtype=torch.int32, device="cuda")
    again = search(600, lens, False, rev=rev, rev_counts=counts, rev_status=rev_status)
    ops.reverse_finish_many([(rev, counts, 600, 600)], rev_status)
    assert torch.equal(again, full)
    want = ops.reverse_neighbors(full, 600, sort=True)
    w = want.shape[1]
    got = torch.sort(rev, 1).values
    assert torch.equal(got[:, :w], want) and (got[:, w:] == 600).all()
    assert rev_status.cpu().tolist() == [w, 0] and int(counts.abs().sum()) == 0


def test_capacity_padding_kernels(ops):
    src = torch.randint(0, 50, (37, 5), dtype=torch.int32, device="cuda")
    src[::3, 2] = 50                                               # shadow index of the source
    for dt in (torch.int32, torch.int64):
        dst = torch.full((64, 8), -7, dtype=dt, device="cuda")
        ops.pad_index_rows(src.to(dt), 50, dst, 64)
        want = torch.full((64, 8), 64, dtype=dt, device="cuda")
        want[:37, :5] = torch.where(src == 50, torch.full_like(src, 64), src).to(dt)
        assert torch.equal(dst, want)
    pts = torch.randn(37, 3, device="cuda")
    dst, cnt = torch.zeros(64, 3, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
    ops.pad_points(pts, dst, 1e6, cnt)
    assert torch.equal(dst[:37], pts) and (dst[37:] == 1e6).all() and int(cnt) == 37
    with pytest.raises(RuntimeError):
        ops.pad_index_rows(src, 50, torch.zeros((20, 8), dtype=torch.int32, device="cuda"), 20)     # too few rows


# ------------------------------------------------------------------ KPConv

KP_CASES = [("g4_kpconv_config1", "linear", "sum"), ("g4_kpconv_gaussian", "gaussian", "sum"),
            ("g4_kpconv_constant", "constant", "sum"), ("g4_kpconv_closest", "linear", "closest"),
            ("g4_kpconv_cin66", "linear", "sum"), ("g4_kpconv_cin2", "linear", "sum"),
            ("g4_kpconv_strided", "linear", "sum")]


@pytest.mark.parametrize("name,influence,agg", KP_CASES)
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_kpconv_fwd_bwd_golden(ops, name, influence, agg, idt):
    g = load_golden(name)
    x = T(g["x"]).requires_grad_(True)
    W = T(g["weights"]).requires_grad_(True)
    y, _ = ops.kpconv(T(g["q"]), T(g["s"]), T(g["idx"]).to(idt), x, T(g["kernel_points"]), W,
                      float(g["extent"]), influence, agg)
    (y * T(g["g"])).sum().backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < FP_TOL
    assert rel_err(x.grad.cpu().numpy(), g["x_grad"]) < FP_TOL
    assert rel_err(W.grad.cpu().numpy(), g["weights_grad"]) < FP_TOL


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_kpconv_config1_literal_radius_degenerate_rows(ops, idt):
    """BASELINE configs[0] read LITERALLY: conv radius r = 0.04 on the 4 096-point lattice of pitch
    0.04 (U(-0.015, 0.015) jitter, 2 cm sine ripple, seed 0), Cin = Cout = 64, K = 15 -- a degenerate neighbourhood of
    1-6 real neighbours per row, 2.7 on average (the point itself, plus the lattice neighbours the jitter pulled inside r), kernel
    extent 0.04 * 1.2 / 2.5 so that most kernel points reach nothing; plus rows emptied completely (all shadow).
    Neighbour rows from the HIP search equal the C oracle's, y / dx / dW equal the float64 NumPy restatement to 1e-4."""
    from oracle import npref, cport
    rng = np.random.default_rng(0)
    ii, jj = np.meshgrid(np.arange(64), np.arange(64), indexing="ij")
    p = np.stack([ii * 0.04, jj * 0.04, 0.02 * np.sin(ii * 0.3)], -1).reshape(-1, 3)
    p = (p + rng.uniform(-0.015, 0.015, p.shape)).astype(np.float32)
    r = 0.04
    lens = np.array([p.shape[0]], np.int32)
    nb = ops.radius_neighbors_batch(T(p), T(p), lens, lens, r)
    want = cport.radius_neighbors_batch(p, p, lens, lens, r)
    assert_neighbors_equal_mod_ties(nb.cpu().numpy(), want, p, p, lens, lens)
    counts = (want < p.shape[0]).sum(1)
    assert counts.min() >= 1 and counts.max() <= 6 and 1.0 < counts.mean() < 4.0, (counts.min(), counts.max(), counts.mean())
    idx = want.copy()
    idx[rng.choice(p.shape[0], 37, replace=False)] = p.shape[0]          # empty rows: all shadow
    K, cin, cout = 15, 64, 64
    extent = r * 1.2 / 2.5
    kp = (rng.normal(size=(K, 3)) * (0.66 * r / 2)).astype(np.float32)
    kp[0] = 0.0
    x = rng.normal(size=(p.shape[0], cin)).astype(np.float32)
    W = (rng.normal(size=(K, cin, cout)) * 0.05).astype(np.float32)
    g = rng.normal(size=(p.shape[0], cout)).astype(np.float32)
    xt, Wt = T(x).requires_grad_(True), T(W).requires_grad_(True)
    y, _ = ops.kpconv(T(p), T(p), T(idx).to(idt), xt, T(kp), Wt, extent)
    (y * T(g)).sum().backward()
    a64 = [p.astype(np.float64), p.astype(np.float64), idx.astype(np.int64), x.astype(np.float64), kp.astype(np.float64),
           W.astype(np.float64), extent]
    yr = npref.kpconv_forward(*a64)
    assert np.abs(yr[(idx >= p.shape[0]).all(1)]).max() == 0.0                    # empty rows convolve to exactly zero
    assert np.array_equal(y.detach().cpu().numpy()[(idx >= p.shape[0]).all(1)], yr[(idx >= p.shape[0]).all(1)].astype(np.float32))
    check_err("config 1 literal r=0.04: y", rel_err(y.detach().cpu().numpy(), yr), FP_TOL)
    dx, dW = npref.kpconv_backward(*a64, g.astype(np.float64))
    check_err("config 1 literal r=0.04: dx", rel_err(xt.grad.cpu().numpy(), dx), FP_TOL)
    check_err("config 1 literal r=0.04: dW", rel_err(Wt.grad.cpu().numpy(), dW), FP_TOL)


VARIANT_SHAPES = [(1, 5, 9), (4, 32, 17), (8, 8, 70), (20, 12, 33), (68, 64, 40),
                  (128, 16, 25), (256, 8, 64), (512, 4, 10), (516, 4, 6), (1040, 3, 5),
                  (2, 6, 130), (130, 16, 150), (600, 4, 130), (30, 5, 260),
                  (61, 8, 40), (62, 8, 16), (67, 8, 33), (129, 8, 20), (255, 4, 70)]
# (linear, sum) runs on the MFMA gather wherever it can; the other two modes run on kpconv_lane_channel (any Cin)
VARIANT_MODES = [("linear", "sum"), ("gaussian", "sum"), ("linear", "closest")]


@pytest.mark.parametrize("cin,cout,H,influence,agg", [
    pytest.param(*shape, *mode, id="-".join(str(v) for v in (shape if mode == VARIANT_MODES[0] else shape + mode)))
    for mode in VARIANT_MODES for shape in VARIANT_SHAPES])
def test_kpconv_every_kernel_variant_vs_numpy_oracle(ops, cin, cout, H, influence, agg):
    """Seeded inputs through every gather / scatter template instantiation (the MFMA gather's tile counts under
    linear / sum; NSLOT = 1, 2, 4, 8 of the generic lane = channel kernel and its > 512-channel multi-launch path as the
    forward under the gaussian influence and the `closest` aggregation, rows of <= 4 channels included, and as the
    scatter; the four-waves-per-point scatter of rows with more than 64 neighbour columns) against the float64
    numpy restatement; includes shadow neighbours, empty rows and a ragged last chunk."""
    from oracle import npref
    rng = np.random.default_rng(cin * 131 + H)
    Nq, Ns, K = 257, 301, 15
    q = (rng.random((Nq, 3)) * 0.3).astype(np.float32)
    s = (rng.random((Ns, 3)) * 0.3).astype(np.float32)
    idx = rng.integers(0, Ns + 1, (Nq, H)).astype(np.int32)
    idx[5] = Ns                                   # a row of shadow neighbours only
    idx[:, H // 2:][rng.random((Nq, H - H // 2)) < 0.5] = Ns
    x = rng.normal(size=(Ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(K, 3)) * 0.05).astype(np.float32)
    W = (rng.normal(size=(K, cin, cout)) * 0.1).astype(np.float32)
    g = rng.normal(size=(Nq, cout)).astype(np.float32)
    xt, Wt = T(x).requires_grad_(True), T(W).requires_grad_(True)
    y, _ = ops.kpconv(T(q), T(s), T(idx), xt, T(kp), Wt, 0.06, influence, agg)
    (y * T(g)).sum().backward()
    a64 = [a.astype(np.float64) for a in (q, s)] + [idx.astype(np.int64), x.astype(np.float64), kp.astype(np.float64),
                                                     W.astype(np.float64), 0.06]
    assert rel_err(y.detach().cpu().numpy(), npref.kpconv_forward(*a64, influence, agg)) < FP_TOL
    dx, dW = npref.kpconv_backward(*a64, g.astype(np.float64), influence, agg)
    assert rel_err(xt.grad.cpu().numpy(), dx) < FP_TOL
    assert rel_err(Wt.grad.cpu().numpy(), dW) < FP_TOL


@pytest.mark.parametrize("cin,H", [(20, 70), (61, 150), (300, 70), (100, 70), (200, 40)])
def test_kpconv_deformable_gather_closest_vs_numpy_oracle(ops, cin, H):
    """Deformable layers with the `closest` aggregation run on kpconv_lane_channel<NSLOT, .., fwd, DEFORM> (the MFMA
    gather takes linear / sum only): NSLOT 1 (20 and 61 channels: a partly filled slot), 8 (300), 2 (100) and 4 (200),
    rows of one, two and three 64-column chunks with a ragged last one.
    Aggregate and min_d2 (over real and shadow entries) against the float64 numpy restatement; linear influence, where
    the reference's in-range filter drops weights that are exactly zero."""
    from oracle import npref
    rng = np.random.default_rng(cin * 131 + H)
    Nq, Ns, K, ext = 50, 301, 15, 0.06
    q = (rng.random((Nq, 3)) * 0.3).astype(np.float32)
    s = (rng.random((Ns, 3)) * 0.3).astype(np.float32)
    idx = rng.integers(0, Ns + 1, (Nq, H)).astype(np.int32)
    idx[:, H // 2:][rng.random((Nq, H - H // 2)) < 0.5] = Ns
    idx[5] = Ns                                   # a row of shadow neighbours only
    x = rng.normal(size=(Ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(K, 3)) * 0.05).astype(np.float32)
    off = (rng.normal(size=(Nq, K, 3)) * 0.02).astype(np.float32)
    A, min_d2 = ops.kpconv_gather(T(q), T(s), T(idx), T(x), T(kp), ext, aggregation="closest", offsets=T(off),
                                  want_min_d2=True)
    a64 = [a.astype(np.float64) for a in (q, s)] + [idx.astype(np.int64), x.astype(np.float64), kp.astype(np.float64)]
    _, want, _ = npref.kpconv_forward(*a64, np.zeros((K, cin, 1)), ext, aggregation="closest",
                                      offsets=off.astype(np.float64), return_A=True)
    assert rel_err(A.cpu().numpy(), want) < FP_TOL
    _, d2 = npref.kpconv_weights(a64[0], a64[1], a64[2], a64[4], ext, aggregation="closest", offsets=off.astype(np.float64))
    want_min = d2.min(axis=1)
    got_min = min_d2.cpu().numpy()
    real = (idx < Ns).any(1)                      # (the all-shadow row's minima are ~3e12: compared on their own scale)
    assert rel_err(got_min[real], want_min[real]) < FP_TOL
    assert rel_err(got_min[~real], want_min[~real]) < FP_TOL


@pytest.mark.parametrize("Nq,cin,H", [(40000, 32, 12), (70000, 66, 30), (17000, 64, 40), (21000, 128, 70), (19000, 66, 40),
                                      (17500, 65, 20)])
def test_kpconv_gather_large_launches_vs_numpy_oracle(ops, Nq, cin, H):
    """Launches of tens of thousands of points on the MFMA gather (one wave per point): the aggregate of every region
    of the launch -- its first rows, the rows an eighth of the way in, the ragged last workgroup, random rows; shadow
    entries in the middle of rows -- against the float64 numpy restatement."""
    from oracle import npref
    rng = np.random.default_rng(Nq + cin)
    Ns, K = 3000, 15
    q = (rng.random((Nq, 3)) * 0.3).astype(np.float32)
    s = (rng.random((Ns, 3)) * 0.3).astype(np.float32)
    idx = rng.integers(0, Ns + 1, (Nq, H)).astype(np.int32)
    idx[:, H // 2:][rng.random((Nq, H - H // 2)) < 0.4] = Ns
    x = rng.normal(size=(Ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(K, 3)) * 0.05).astype(np.float32)
    A = ops.kpconv_gather(T(q), T(s), T(idx), T(x), T(kp), 0.06)[0].cpu().numpy()
    eighth = (Nq // 8) * 4
    rows = np.unique(np.concatenate([np.arange(0, 64), np.arange(eighth - 64, eighth + 64),
                                     np.arange(Nq - 64, Nq), rng.integers(0, Nq, 512)]))
    W1 = np.zeros((K, cin, 1))
    _, want, _ = npref.kpconv_forward(q[rows].astype(np.float64), s.astype(np.float64), idx[rows].astype(np.int64),
                                      x.astype(np.float64), kp.astype(np.float64), W1, 0.06, return_A=True)
    assert rel_err(A[rows], want) < FP_TOL


@pytest.mark.parametrize("Nq,cin,H", [(3001, 64, 30), (19000, 66, 40), (21000, 128, 30), (9000, 300, 20), (5000, 3, 20)])
def test_kpconv_gather_with_a_work_list_writes_the_rows_of_the_plain_gather(ops, Nq, cin, H):
    """mvk_kpconv_gather_fwd_ordered: the work list only changes which wave (and which XCD) works on a point. Every
    point is summed in the same way whatever its slot, so every work list must give the same BITS as the row order;
    the layer as a whole (ops.kpconv) to 2e-6."""
    rng = np.random.default_rng(Nq + cin)
    Ns, K = Nq, 15
    s = (rng.random((Ns, 3)) * 0.6).astype(np.float32)
    q = s
    idx = rng.integers(0, Ns + 1, (Nq, H)).astype(np.int32)
    idx[:, H // 2:][rng.random((Nq, H - H // 2)) < 0.4] = Ns
    x = T(rng.normal(size=(Ns, cin)).astype(np.float32))
    kp = T((rng.normal(size=(K, 3)) * 0.05).astype(np.float32))
    qt, st, it = T(q), T(s), T(idx)
    plain = ops.kpconv_gather(qt, st, it, x, kp, 0.06)[0]
    cells = np.floor(s / 0.06).astype(np.int64)
    orders = {"random": rng.permutation(Nq), "reversed": np.arange(Nq)[::-1].copy(),
              "cells": np.lexsort((cells[:, 0], cells[:, 1], cells[:, 2]))}
    for name, o in orders.items():
        got = ops.kpconv_gather(qt, st, it, x, kp, 0.06, order=T(o.astype(np.int32)))[0]
        assert torch.equal(got, plain), (name, Nq, cin)
    with pytest.raises(RuntimeError):
        ops.kpconv_gather(qt, st, it, x, kp, 0.06, order=T(np.arange(Nq - 1, dtype=np.int32)))
    if cin == 66:
        W = T((rng.normal(size=(K, cin, 32)) * 0.1).astype(np.float32))
        y0 = ops.kpconv(qt, st, it, x, kp, W, 0.06)[0]
        y1 = ops.kpconv(qt, st, it, x, kp, W, 0.06, order=T(orders["cells"].astype(np.int32)))[0]
        check_err("KPConv layer with a work list vs without", float((y1 - y0).abs().max() / y0.abs().max()), 2e-6)


@pytest.mark.parametrize("C1,C2,idt", [(256, 128, torch.int32), (30, 7, torch.int64), (64, 64, torch.int32)])
def test_upsample_cat_equals_closest_pool_then_cat(ops, C1, C2, idt):
    """mvk_gather_rows_cat_fwd: [closest_pool(x, inds) | skip] (blocks.py:79-91 + architectures.py:334) in one launch --
    the same bits as the two steps, shadow rows included, and the same gradients for both inputs."""
    rng = np.random.default_rng(C1 + C2)
    Ns, Nq, H = 700, 2900, 5
    inds = T(rng.integers(0, Ns + 1, (Nq, H))).to(idt)
    x = T(rng.normal(size=(Ns, C1)).astype(np.float32)).requires_grad_(True)
    skip = T(rng.normal(size=(Nq, C2)).astype(np.float32)).requires_grad_(True)
    x2, skip2 = x.detach().clone().requires_grad_(True), skip.detach().clone().requires_grad_(True)
    g = T(rng.normal(size=(Nq, C1 + C2)).astype(np.float32))
    got = ops.upsample_cat(x, inds, skip)
    want = torch.cat([ops.closest_pool(x2, inds), skip2], dim=1)
    assert torch.equal(got, want)
    ops.step_begin()
    (got * g).sum().backward()
    (want * g).sum().backward()
    assert torch.equal(skip.grad, skip2.grad)
    assert rel_err(x.grad.cpu().numpy(), x2.grad.cpu().numpy()) < 1e-6       # float atomics: order of arrival


@pytest.mark.parametrize("R,Da,Db,from_gemm", [(85, 128, 512, False), (700, 64, 256, False), (700, 30, 64, False),
                                               (5000, 32, 128, False), (5000, 64, 128, True), (19464, 32, 128, True)])
def test_bn_lrelu_pair_equals_two_single_launches(ops, R, Da, Db, from_gemm):
    """mvk_bn_lrelu_fwd_pair / _bwd_pair: the same kernels, two problems per launch (the convolution output and the
    shortcut of a bottleneck block) -- outputs, running statistics, batch counters and all gradients bit-identical to
    two calls of bn_lrelu, in every kernel family (one workgroup per channel group <= 128 rows, register-resident
    <= 1024 rows, two-stage above; statistics from the producing GEMM's epilogue or from the extra pass), capacity
    padding included."""
    rng = np.random.default_rng(R + Da)
    n_valid = T(np.asarray([R - 37 if R > 100 else R], np.int32))

    def make():
        torch.manual_seed(1)
        bns = [torch.nn.BatchNorm1d(D, momentum=0.02).cuda().train() for D in (Da, Db)]
        for bn in bns:
            bn.weight.data.uniform_(0.5, 1.5)
            bn.bias.data.uniform_(-0.3, 0.3)
        return bns

    if from_gemm:       # inputs that carry the epilogue statistics of the GEMM that made them
        A = T(rng.normal(size=(R, 96)).astype(np.float32))
        Wa, Wb = T(rng.normal(size=(Da, 96)).astype(np.float32)), T(rng.normal(size=(Db, 96)).astype(np.float32))
        inputs = lambda: (ops.linear(A, Wa, stats_n_valid=n_valid), ops.linear(A, Wb, stats_n_valid=n_valid))
    else:
        Xa, Xb = T(rng.normal(size=(R, Da)).astype(np.float32)), T(rng.normal(size=(R, Db)).astype(np.float32) * 3 + 1)
        inputs = lambda: (Xa.clone(), Xb.clone())
    ga, gb = T(rng.normal(size=(R, Da)).astype(np.float32)), T(rng.normal(size=(R, Db)).astype(np.float32))

    bn1 = make()
    xa, xb = [t.detach().requires_grad_(True) for t in inputs()]
    xa._mvk_bn_stats, xb._mvk_bn_stats = [getattr(t, "_mvk_bn_stats", None) for t in inputs()] if from_gemm else (None, None)
    ya = ops.bn_lrelu(xa, n_valid, bn1[0], 0.1)
    yb = ops.bn_lrelu(xb, n_valid, bn1[1], 1.0)
    ((ya * ga).sum() + (yb * gb).sum()).backward()

    bn2 = make()
    pa, pb = [t.detach().requires_grad_(True) for t in inputs()]
    pa._mvk_bn_stats, pb._mvk_bn_stats = [getattr(t, "_mvk_bn_stats", None) for t in inputs()] if from_gemm else (None, None)
    za, zb = ops.bn_lrelu_pair(pa, bn2[0], 0.1, pb, bn2[1], 1.0, n_valid)
    ((za * ga).sum() + (zb * gb).sum()).backward()

    assert torch.equal(za, ya) and torch.equal(zb, yb)
    assert torch.equal(pa.grad, xa.grad) and torch.equal(pb.grad, xb.grad)
    for m1, m2 in zip(bn1, bn2):
        assert torch.equal(m1.running_mean, m2.running_mean) and torch.equal(m1.running_var, m2.running_var)
        assert int(m1.num_batches_tracked) == int(m2.num_batches_tracked) == 1
        assert torch.equal(m1.weight.grad, m2.weight.grad) and torch.equal(m1.bias.grad, m2.bias.grad)


def off_by_one_float(t):
    """A contiguous copy of t whose storage starts one float past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 1, device=t.device, dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def test_bn_lrelu_pair_with_one_misaligned_problem_equals_two_single_launches(ops):
    """Two problems of 300 rows (the register-resident family) whose second input, and its upstream gradient, start one
    float past a 16-byte boundary: that problem cannot take the float4 kernels, the two fall into different families
    and the pair runs as two single dispatches -- still bit-identical to two calls of bn_lrelu."""
    R, Da, Db = 300, 64, 128
    rng = np.random.default_rng(R + Da)
    n_valid = T(np.asarray([R - 37], np.int32))
    Xa, Xb = T(rng.normal(size=(R, Da)).astype(np.float32)), T(rng.normal(size=(R, Db)).astype(np.float32) * 3 + 1)
    ga, gb = T(rng.normal(size=(R, Da)).astype(np.float32)), off_by_one_float(T(rng.normal(size=(R, Db)).astype(np.float32)))

    def make():
        torch.manual_seed(1)
        bns = [torch.nn.BatchNorm1d(D, momentum=0.02).cuda().train() for D in (Da, Db)]
        for bn in bns:
            bn.weight.data.uniform_(0.5, 1.5)
            bn.bias.data.uniform_(-0.3, 0.3)
        return bns

    bn1 = make()
    xa, xb = Xa.clone().requires_grad_(True), off_by_one_float(Xb).requires_grad_(True)
    ya = ops.bn_lrelu(xa, n_valid, bn1[0], 0.1)
    yb = ops.bn_lrelu(xb, n_valid, bn1[1], 1.0)
    torch.autograd.backward([ya, yb], [ga, gb])
    bn2 = make()
    pa, pb = Xa.clone().requires_grad_(True), off_by_one_float(Xb).requires_grad_(True)
    za, zb = ops.bn_lrelu_pair(pa, bn2[0], 0.1, pb, bn2[1], 1.0, n_valid)
    torch.autograd.backward([za, zb], [ga, gb])
    assert torch.equal(za, ya) and torch.equal(zb, yb) and (zb[R - 37:] == 0).all()
    assert torch.equal(pa.grad, xa.grad) and torch.equal(pb.grad, xb.grad)
    for m1, m2 in zip(bn1, bn2):
        assert torch.equal(m1.running_mean, m2.running_mean) and torch.equal(m1.running_var, m2.running_var)
        assert int(m1.num_batches_tracked) == int(m2.num_batches_tracked) == 1
        assert torch.equal(m1.weight.grad, m2.weight.grad) and torch.equal(m1.bias.grad, m2.bias.grad)


@pytest.mark.parametrize("M,Kd,N0,N1,stats", [(4288, 128, 64, 256, True), (332, 512, 256, 1024, False),
                                              (85, 1024, 512, 2048, False), (19464, 64, 32, 128, True), (1300, 256, 128, 512, True)])
def test_linear_pair_equals_two_linear_layers(ops, M, Kd, N0, N1, stats):
    """mvk_gemm_f32_pair: unary1 and the shortcut layer of a bottleneck block (same input) as one launch -- outputs,
    epilogue statistics and all three gradients against two ops.linear calls (unsplit products: the same bits; split
    ones: the rounding of the atomics' order)."""
    rng = np.random.default_rng(M + N0)
    x = T(rng.normal(size=(M, Kd)).astype(np.float32)).requires_grad_(True)
    W0 = T((rng.normal(size=(N0, Kd)) * 0.1).astype(np.float32)).requires_grad_(True)
    W1 = T((rng.normal(size=(N1, Kd)) * 0.1).astype(np.float32)).requires_grad_(True)
    nv = T(np.asarray([M - 5], np.int32)) if stats else None
    x2, V0, V1 = [t.detach().clone().requires_grad_(True) for t in (x, W0, W1)]
    g0, g1 = T(rng.normal(size=(M, N0)).astype(np.float32)), T(rng.normal(size=(M, N1)).astype(np.float32))
    pair = ops.linear_pair(x, W0, W1, nv)       # (N0 = 32: the narrow product rides on its partner's wide tiles)
    y0, y1 = pair
    r0, r1 = ops.linear(x2, V0, stats_n_valid=nv), ops.linear(x2, V1, stats_n_valid=nv)
    for a, b_ in ((y0, r0), (y1, r1)):
        assert rel_err(a.detach().cpu().numpy(), b_.detach().cpu().numpy()) < 2e-6
        sa, sb = ops.bn_stats_of(a), ops.bn_stats_of(b_)
        assert (sa is None) == (sb is None)
        if sa is not None:
            assert sa[1] == sb[1] and rel_err(sa[0].detach().cpu().numpy(), sb[0].detach().cpu().numpy()) < 2e-6
    ((y0 * g0).sum() + (y1 * g1).sum()).backward()
    ((r0 * g0).sum() + (r1 * g1).sum()).backward()
    assert rel_err(x.grad.cpu().numpy(), x2.grad.cpu().numpy()) < 2e-6
    assert rel_err(W0.grad.cpu().numpy(), V0.grad.cpu().numpy()) < 2e-6
    assert rel_err(W1.grad.cpu().numpy(), V1.grad.cpu().numpy()) < 2e-6


@pytest.mark.parametrize("M,Kd,N,slope", [(19464, 128, 128, 0.1), (19464, 128, 20, 1.0), (333, 64, 7, 0.1), (5, 256, 256, 0.2)])
def test_linear_bias_lrelu_equals_linear_then_bias_lrelu(ops, M, Kd, N, slope):
    """mvk_gemm_f32_bias_act: the BatchNorm-less head layers (x W^T + bias, LeakyReLU; blocks.py:462-463) with bias and
    activation in the GEMM's store -- outputs and the three gradients against ops.linear + ops.bias_lrelu."""
    rng = np.random.default_rng(M + N)
    x = T(rng.normal(size=(M, Kd)).astype(np.float32)).requires_grad_(True)
    W = T((rng.normal(size=(N, Kd)) * 0.1).astype(np.float32)).requires_grad_(True)
    b = T(rng.normal(size=(N,)).astype(np.float32)).requires_grad_(True)
    x2, W2, b2 = [t.detach().clone().requires_grad_(True) for t in (x, W, b)]
    g = T(rng.normal(size=(M, N)).astype(np.float32))
    y = ops.linear_bias_lrelu(x, W, b, slope)
    r = ops.bias_lrelu(ops.linear(x2, W2), b2, slope)
    assert rel_err(y.detach().cpu().numpy(), r.detach().cpu().numpy()) < 2e-6
    ops.step_begin()
    (y * g).sum().backward()
    (r * g).sum().backward()
    for a, c in ((x, x2), (W, W2), (b, b2)):
        assert rel_err(a.grad.cpu().numpy(), c.grad.cpu().numpy()) < 5e-6


@pytest.mark.parametrize("M,N,Kd,Kd2", [(4288, 128, 64, 256), (85, 1024, 512, 2048), (332, 512, 256, 1024), (19464, 64, 32, 128),
                                        (1300, 256, 128, 500), (700, 128, 48, 64), (700, 20, 64, 64)])
def test_gemm_dual_equals_the_sum_of_two_products(ops, M, N, Kd, Kd2):
    """mvk_gemm_f32_dual: A B + A2 B2 with the reductions laid end to end (every split of the concatenated reduction,
    ragged second reduction included) against two float64 products; None for the shapes it does not take (a first
    reduction that is not a whole number of k-tiles, outputs of <= 32 columns)."""
    rng = np.random.default_rng(M + N + Kd2)
    A, B = rng.normal(size=(M, Kd)).astype(np.float32), (rng.normal(size=(Kd, N)) * 0.1).astype(np.float32)
    A2, B2 = rng.normal(size=(M, Kd2)).astype(np.float32), (rng.normal(size=(Kd2, N)) * 0.1).astype(np.float32)
    ops.step_begin()
    got = ops.gemm_dual(T(A), T(B), T(A2), T(B2))
    if Kd % 32 != 0 or N <= 32:
        assert got is None
        return
    want = A.astype(np.float64) @ B.astype(np.float64) + A2.astype(np.float64) @ B2.astype(np.float64)
    assert rel_err(got.cpu().numpy(), want) < 2e-6


@pytest.mark.parametrize("Ns,Nq,C1,C2,Cout,idt", [(1300, 4288, 512, 256, 256, torch.int32), (85, 332, 2048, 1024, 1024, torch.int32),
                                                   (4288, 19464, 256, 128, 128, torch.int64), (300, 1000, 30, 7, 16, torch.int32)])
def test_upsample_cat_linear_equals_the_three_steps(ops, Ns, Nq, C1, C2, Cout, idt):
    """closest_pool + torch.cat + nn.Linear of the decoder as one autograd node whose backward is ONE product with a
    scatter epilogue (mvk_gemm_f32_scatter_cat): output and the gradients of the coarse features, the skip features and
    the weight against the three separate steps (split and unsplit plans, shadow indices, both index widths)."""
    rng = np.random.default_rng(Ns + C1)
    inds = T(rng.integers(0, Ns + 1, (Nq, 4))).to(idt)
    x = T(rng.normal(size=(Ns, C1)).astype(np.float32)).requires_grad_(True)
    skip = T(rng.normal(size=(Nq, C2)).astype(np.float32)).requires_grad_(True)
    W = T((rng.normal(size=(Cout, C1 + C2)) * 0.05).astype(np.float32)).requires_grad_(True)
    x2, skip2, W2 = [t.detach().clone().requires_grad_(True) for t in (x, skip, W)]
    g = T(rng.normal(size=(Nq, Cout)).astype(np.float32))
    ops.step_begin()
    y = ops.upsample_cat_linear(x, inds, skip, W)
    r = ops.linear(torch.cat([ops.closest_pool(x2, inds), skip2], dim=1), W2)
    assert rel_err(y.detach().cpu().numpy(), r.detach().cpu().numpy()) < 2e-6
    (y * g).sum().backward()
    (r * g).sum().backward()
    for a, c in ((x, x2), (skip, skip2), (W, W2)):
        assert rel_err(a.grad.cpu().numpy(), c.grad.cpu().numpy()) < 5e-6


def test_cell_order_of_the_neighbour_search_is_a_sorted_permutation(ops):
    """mvk_neighbors_cell_order after a radius search over three stacked clouds: a permutation of the rows that stays
    inside each cloud, ascending in the grid cell of the search (cell = 1.001 r from the cloud's minimum corner,
    x fastest) and in the row inside a cell, identical on a second call, identity over the capacity padding."""
    rng = np.random.default_rng(77)
    lens = np.asarray([4000, 1, 2500], np.int32)
    pts = np.concatenate([(rng.random((n, 3)) * (0.8 + 0.3 * i)).astype(np.float32) + 5.0 * i for i, n in enumerate(lens)])
    r = 0.1
    P = T(pts)
    nb = ops.radius_neighbors_batch(P, P, lens, lens, r, limit=20)
    assert nb.shape == (len(pts), 20)
    cap = len(pts) + 100
    out = torch.full((cap,), -7, dtype=torch.int32, device=P.device)
    ops.neighbors_cell_order(len(pts), len(pts), 3, out)
    again = ops.neighbors_cell_order(len(pts), len(pts), 3, device=P.device)
    o = out.cpu().numpy()
    assert np.array_equal(o[len(pts):], np.arange(len(pts), cap)) and np.array_equal(o[:len(pts)], again.cpu().numpy())
    _check_cell_order(o, pts, lens, r)


def _check_cell_order(o, pts, lens, r):
    off = 0
    for n in lens:
        if n == 0:
            continue
        seg = o[off:off + n].astype(np.int64)
        assert np.array_equal(np.sort(seg), np.arange(off, off + n))
        p = pts[seg]
        lo = pts[off:off + n].min(0)
        cell = np.float32(r) * np.float32(1.001)
        c = np.floor((p - lo) / cell).astype(np.int64)
        d = np.floor((pts[off:off + n].max(0) - lo) / cell).astype(np.int64) + 1
        lin = (c[:, 2] * d[1] + c[:, 1]) * d[0] + c[:, 0]
        key = lin * (1 << 32) + seg
        assert np.all(np.diff(key) > 0)
        off += n


def test_cell_order_with_crowded_cells(ops):
    """Cells of 17-64 rows (ranked by a wavefront, one lane per row) and of more than 64 rows (64 at a time against all),
    in runs of neighbouring cells and next to empty ones, two clouds of which the second starts mid-wavefront."""
    rng = np.random.default_rng(78)
    r = 0.1
    blobs = []
    for k, n in enumerate((17, 33, 64, 65, 200, 31, 16, 129)):              # rows per crowded cell
        centre = np.asarray([0.05 + 0.1003 * k, 0.05, 0.05], np.float32)     # neighbouring cells along x
        blobs.append(centre + (rng.random((n, 3)).astype(np.float32) - 0.5) * 0.02)
    sparse = (rng.random((3000, 3)) * [2.0, 1.0, 0.5]).astype(np.float32)
    a = np.concatenate(blobs + [sparse])
    a = a[rng.permutation(len(a))]
    b = np.concatenate([blobs[4] + 3.0, (rng.random((700, 3)) * 0.7).astype(np.float32) + 3.0])
    b = b[rng.permutation(len(b))]
    pts = np.ascontiguousarray(np.concatenate([a, b]), np.float32)
    lens = np.asarray([len(a), len(b)], np.int32)
    P = T(pts)
    ops.radius_neighbors_batch(P, P, lens, lens, r, limit=8)
    o = ops.neighbors_cell_order(len(pts), len(pts), 2, device=P.device).cpu().numpy()
    _check_cell_order(o, pts, lens, r)


def test_neighbors_grid_of_more_than_one_scan_pass(ops):
    """A support grid of more than 65 536 cells (the scan kernel of the multi-workgroup build takes 65 536 cells per pass
    of its workgroup) beside a small cloud and an empty one: rows vs the CPU port, cell order a sorted permutation."""
    from oracle import cport
    rng = np.random.default_rng(79)
    big = (rng.random((30000, 3)) * [3.0, 3.0, 1.3]).astype(np.float32)      # 0.05 cells: 60 x 60 x 26 = 93 600
    small = (rng.random((900, 3)) * 0.4).astype(np.float32) + 7.0
    s = np.concatenate([big, small])
    sl = np.asarray([30000, 0, 900], np.int32)
    q = np.concatenate([big[:3000], small[:200]])
    ql = np.asarray([3000, 0, 200], np.int32)
    r = 0.05
    want = cport.radius_neighbors_batch(q, s, ql, sl, r)
    got = ops.radius_neighbors_batch(T(q), T(s), ql, sl, r).cpu().numpy()
    assert got.shape == want.shape and np.array_equal(got, want)
    S = T(s)
    ops.radius_neighbors_batch(S, S, sl, sl, r, limit=4)
    o = ops.neighbors_cell_order(len(s), len(s), 3, device=S.device).cpu().numpy()
    _check_cell_order(o, s, sl, r)


def test_input_kernels_on_both_paths_at_every_size():
    """The subsampling and neighbour suites once more in child processes with the multi-workgroup front ends forced for
    every cloud (thresholds 1: empty, one-point and ragged clouds included) and switched off (0): the two paths of
    csrc/subsample.hip and csrc/neighbors.hip give the same bits as the goldens and the CPU port whatever the size."""
    import subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    for thr in ("1", "0"):
        env = dict(os.environ, MVK_SUB_MULTI_MIN=thr, MVK_NB_MULTI_MIN=thr, MVK_PARITY_LOG=os.devnull,
                   MVK_NB_WIDE_WAVES="8" if thr == "1" else "1")      # (rows of > 64 columns: eight wavefronts per query / one)
        r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu", "-p", "no:cacheprovider",
                            os.path.join(here, "test_gpu_parity.py"), os.path.join(here, "test_gpu_golden_pipeline.py"),
                            "-k", "(subsample or neighbors or cell_order or pyramid or scene_load) and not both_paths"],
                           env=env, cwd=os.path.dirname(here), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, "thresholds %s:\n%s" % (thr, (r.stdout + r.stderr)[-3000:])
        assert " passed" in r.stdout and "failed" not in r.stdout


@pytest.mark.parametrize("use_rev", [False, True])
@pytest.mark.parametrize("name,modulated", [("g4_kpconv_deform", False), ("g4_kpconv_deform_mod", True)])
def test_kpconv_deformable_golden(ops, name, modulated, use_rev):
    """The reference's deformable (and modulated) KPConv, forward and every gradient (fixture G4 from models.blocks.KPConv).
    use_rev: the feature gradient of BOTH convolutions -- the inner rigid one that makes the offsets (45 / 60 output
    channels) and the deformable one -- as gathers over the transposed neighbourhood relation (round 5:
    mvk_kpconv_gather_rev_deform with the kernel points and modulations of the neighbour rows) instead of the atomic
    scatter; same fixture, same tolerance."""
    g = load_golden(name)
    K = 15
    q, s, idx = T(g["q"]), T(g["s"]), T(g["idx"])
    x = T(g["x"]).requires_grad_(True)
    W = T(g["weights"]).requires_grad_(True)
    Wo = T(g["offset_weights"]).requires_grad_(True)
    bo = T(g["offset_bias"]).requires_grad_(True)
    ext = float(g["extent"])
    rev = ops.reverse_neighbors(idx, s.shape[0]) if use_rev else None
    feat, _ = ops.kpconv(q, s, idx, x, T(g["offset_kernel_points"]), Wo, ext, rev=rev)
    feat = feat + bo
    if modulated:
        off = feat[:, :3 * K].reshape(-1, K, 3) * ext
        mod = 2 * torch.sigmoid(feat[:, 3 * K:])
    else:
        off, mod = feat.reshape(-1, K, 3) * ext, None
    y, min_d2 = ops.kpconv(q, s, idx, x, T(g["kernel_points"]), W, ext, offsets=off, modulations=mod, rev=rev)
    dKP = off + T(g["kernel_points"])
    loss = (y * T(g["g"])).sum() + (min_d2.sum() + (dKP ** 2).sum()) * 0.5
    loss.backward()
    assert rel_err(y.detach().cpu().numpy(), g["y"]) < FP_TOL
    assert rel_err(min_d2.detach().cpu().numpy(), g["min_d2"]) < FP_TOL
    assert rel_err(dKP.detach().cpu().numpy(), g["deformed_KP"]) < FP_TOL
    assert rel_err(W.grad.cpu().numpy(), g["weights_grad"]) < FP_TOL
    # offset path (sqrt' / sigmoid chain through the inner KPConv): measured errors are recorded, bound = DEFORM_TOL
    check_err("G4 %s x_grad" % name, rel_err(x.grad.cpu().numpy(), g["x_grad"]), DEFORM_TOL)
    check_err("G4 %s offset_weights_grad" % name, rel_err(Wo.grad.cpu().numpy(), g["offset_weights_grad"]), DEFORM_TOL)
    check_err("G4 %s offset_bias_grad" % name, rel_err(bo.grad.cpu().numpy(), g["offset_bias_grad"]), DEFORM_TOL)


def test_kpconv_linearity_full_size(ops):
    """BASELINE-size property: KPConv is linear in x and in W (20k points, Cin=Cout=64)."""
    rng = np.random.default_rng(1)
    raw = (rng.random((300000, 3)) * [2.4, 2.4, 0.05]).astype(np.float32)
    p, l = ops.grid_subsample_batch(T(raw), [raw.shape[0]], dl=0.04)
    nb = ops.radius_neighbors_batch(p, p, l, l, 0.1, limit=40)
    g = load_golden("g4_kpconv_config1")
    kp, W = T(g["kernel_points"]), T(g["weights"])
    x1, x2 = torch.randn(p.shape[0], 64, device="cuda"), torch.randn(p.shape[0], 64, device="cuda")
    f = lambda x, w: ops.kpconv(p, p, nb, x, kp, w, 0.048)[0]
    a = f(x1 * 2 - x2 * 3, W)
    b = 2 * f(x1, W) - 3 * f(x2, W)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < FP_TOL
    assert rel_err(f(x1, W * 0.5).cpu().numpy(), (0.5 * f(x1, W)).cpu().numpy()) < FP_TOL


def test_deformable_offset_gradient_properties_full_size(ops):
    """BASELINE-size properties of the deformable backward (config 5 geometry: a level of ~3 500 points, ~250 neighbour
    columns at the deform radius, Cin 128): d_offsets is linear in the upstream gradient, it vanishes with it, and it
    equals the finite-difference slope of the forward along a random offset direction (central difference in float64
    of the float32 forward, 2 % -- the forward is piecewise smooth in the offsets)."""
    rng = np.random.default_rng(11)
    raw = (rng.random((200000, 3)) * [4.8, 4.8, 0.8]).astype(np.float32)
    p, l = ops.grid_subsample_batch(T(raw), [raw.shape[0]], dl=0.16)
    nb = ops.radius_neighbors_batch(p, p, l, l, 0.16 * 6.0, limit=250)
    N = p.shape[0]
    assert N > 1500 and nb.shape[1] >= 100
    K, Cin, Cout, ext = 15, 128, 32, 0.16 * 1.2
    torch.manual_seed(3)
    kp = (torch.rand(K, 3, device="cuda") - 0.5) * 0.5
    kp[0] = 0
    W = torch.randn(K, Cin, Cout, device="cuda") * 0.05
    x = torch.randn(N, Cin, device="cuda")
    off0 = torch.randn(N, K, 3, device="cuda") * 0.03

    def grad_off(gy, gmin):
        off = off0.clone().requires_grad_(True)
        y, md = ops.kpconv(p, p, nb, x, kp, W, ext, offsets=off)
        (gy_, gm_) = (gy, gmin)
        torch.autograd.backward([y, md], [gy_, gm_])
        return off.grad
    g1, g2 = torch.randn(N, Cout, device="cuda"), torch.randn(N, Cout, device="cuda")
    m1, m2 = torch.randn(N, K, device="cuda"), torch.randn(N, K, device="cuda")
    a = grad_off(2 * g1 - 3 * g2, 2 * m1 - 3 * m2)
    b = 2 * grad_off(g1, m1) - 3 * grad_off(g2, m2)
    assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-4
    assert float(grad_off(torch.zeros_like(g1), torch.zeros_like(m1)).abs().max()) == 0.0
    # directional derivative on a subset of points (each point's offsets only influence its own output row)
    d = torch.randn(N, K, 3, device="cuda")
    eps = 2e-3 * ext
    with torch.no_grad():
        yp, mp = ops.kpconv(p, p, nb, x, kp, W, ext, offsets=off0 + eps * d)
        ym, mm = ops.kpconv(p, p, nb, x, kp, W, ext, offsets=off0 - eps * d)
    fd = (((yp.double() - ym.double()) * g1.double()).sum(1) + ((mp.double() - mm.double()) * m1.double()).sum(1)) / (2 * eps)
    an = (grad_off(g1, m1).double() * d.double()).sum((1, 2))
    rel = (fd - an).abs() / (an.abs() + 1e-3 * an.abs().mean())
    # (with ~250 neighbours x 15 kernel points a finite step crosses a clamp / arg-min kink for a minority of the points)
    assert float(rel.median()) < 2e-2 and float((rel < 0.1).float().mean()) > 0.8


def test_pools_golden(ops):
    g = load_golden("g4_pools")
    x, idx = T(g["x"]), T(g["pool_idx"])
    assert bits_equal(ops.max_pool(x, idx).cpu().numpy(), g["max_pool"])
    assert bits_equal(ops.closest_pool(x, idx.long()).cpu().numpy(), g["closest_pool"])
    # backward vs torch autograd restatement of blocks.py:79-110
    xr = T(g["x"]).requires_grad_(True)
    xp = torch.cat([xr, torch.zeros_like(xr[:1])], 0)
    ref = xp[idx.long()].max(1)[0]
    gr = torch.randn_like(ref)
    ref.backward(gr)
    x2 = T(g["x"]).requires_grad_(True)
    ops.max_pool(x2, idx).backward(gr)
    assert rel_err(x2.grad.cpu().numpy(), xr.grad.cpu().numpy()) < 1e-6


# ------------------------------------------------------------------ gemm

@pytest.mark.parametrize("M,N,K", [(64, 64, 16), (100, 45, 990), (4096, 64, 960), (33, 70, 7), (1, 1, 1),
                                   (19464, 32, 480), (300, 20, 129), (130, 7, 990), (990, 32, 4001)])
def test_gemm_f32_mfma(ops, M, N, K):
    """64 x 64 tiles and, for N <= 32, the 128 x 32 tiles; all three operand layouts, with and without split-K."""
    torch.manual_seed(0)
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(K, N, device="cuda") + 0.1 * torch.arange(N, device="cuda")   # asymmetric
    ref = (A.double() @ B.double()).cpu().numpy()
    assert rel_err(ops.gemm(A, B).cpu().numpy(), ref) < 1e-5
    assert rel_err(ops.gemm(A, B.t().contiguous(), transB=True).cpu().numpy(), ref) < 1e-5
    assert rel_err(ops.gemm(A.t().contiguous(), B, transA=True, split_k=3).cpu().numpy(), ref) < 1e-5
    assert rel_err(ops.gemm(A.t().contiguous(), B.t().contiguous(), transA=True, transB=True, split_k=1).cpu().numpy(), ref) < 1e-5


@pytest.mark.parametrize("pm,qn", [(1, 1), (2, 1), (4, 1), (5, 1), (1, 2), (2, 2), (4, 2)])
def test_gemm_f32_every_tile_configuration(ops, pm, qn, monkeypatch):
    """Every (rows per wave, column blocks per wave) instantiation of gemm_f32_mfma, all four operand layouts,
    ragged sizes (M, N, K not multiples of the tile), with and without a split: MVK_GEMM_FORCE pins the plan."""
    torch.manual_seed(pm * 10 + qn)
    M, N, K = 16 * pm * 3 + 7, (150 if qn == 2 else 70), 203
    A = torch.randn(M, K, device="cuda")
    B = torch.randn(K, N, device="cuda") + 0.1 * torch.arange(N, device="cuda")
    ref = (A.double() @ B.double()).cpu().numpy()
    for split in (1, 3):
        monkeypatch.setenv("MVK_GEMM_FORCE", "%d,%d,%d" % (pm, qn, split))
        assert rel_err(ops.gemm(A, B).cpu().numpy(), ref) < 1e-5
        assert rel_err(ops.gemm(A, B.t().contiguous(), transB=True).cpu().numpy(), ref) < 1e-5
        assert rel_err(ops.gemm(A.t().contiguous(), B, transA=True).cpu().numpy(), ref) < 1e-5
        assert rel_err(ops.gemm(A.t().contiguous(), B.t().contiguous(), transA=True, transB=True).cpu().numpy(), ref) < 1e-5
    # narrow outputs (N <= 32: the waves split the rows)
    for n_cols in (20, 32, 9):
        monkeypatch.setenv("MVK_GEMM_FORCE", "%d,0,1" % min(pm, 2))
        Bn = torch.randn(K, n_cols, device="cuda")
        refn = (A.double() @ Bn.double()).cpu().numpy()
        assert rel_err(ops.gemm(A, Bn).cpu().numpy(), refn) < 1e-5
        assert rel_err(ops.gemm(A.t().contiguous(), Bn.t().contiguous(), transA=True, transB=True).cpu().numpy(), refn) < 1e-5


@pytest.mark.parametrize("M,N,K,n", [(19464, 64, 990, 19464), (19464, 32, 480, 19000), (3986, 64, 960, 3986), (1300, 128, 96, 1207),
                                     (4096, 200, 64, 4000), (1100, 256, 64, 1100), (19464, 128, 32, 19464), (5000, 20, 64, 4321)])
def test_gemm_batchnorm_statistics_epilogue(ops, M, N, K, n):
    """The statistics the GEMM epilogue hands to the BatchNorm that follows (per wave row block: column sum and
    centred sum of squares over the rows below n_valid) give the same normalised output, running statistics and
    saved mean / invstd as the separate statistics pass -- and as torch's batch_norm over the valid rows. The mean
    is far from zero (|mean| ~ 50 sigma): a plain E[x^2] - E[x]^2 would lose the variance."""
    torch.manual_seed(M + N)
    A = torch.randn(M, K, device="cuda")
    A[:, 0] = 40.0                                          # large common component -> large column means
    B = torch.randn(K, N, device="cuda")
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    # outputs whose BatchNorm is a single launch anyway (<= 128 rows, <= 1024 when N % 4 == 0) get no statistics
    small = torch.randn(ops.bn_single_launch_rows(N), K, device="cuda")
    assert ops.gemm(small, B, split_k=1, stats_n_valid=nv)[1] is None and ops.bn_single_launch_rows(64) == 1024
    auto, st_auto = ops.gemm(A, B, stats_n_valid=nv)          # the plan may prefer a split reduction (then no statistics)
    assert rel_err(auto.cpu().numpy(), (A.double() @ B.double()).cpu().numpy()) < 1e-5
    assert (st_auto is None) == (ops.gemm_plan(M, N, K, None, True)[1] == 0)
    y, st = ops.gemm(A, B, split_k=1, stats_n_valid=nv)       # unsplit: statistics always come with it
    assert rel_err(y.cpu().numpy(), (A.double() @ B.double()).cpu().numpy()) < 1e-5
    split, rows = ops.gemm_plan(M, N, K, 1, True)
    assert split == 1 and rows > 0 and st is not None
    part, prow = st
    assert prow == rows and part.shape == ((M + rows - 1) // rows, 2, N)
    yv = y[:n].double()
    # partials against float64: block sums and centred sums of squares
    nb = (n + rows - 1) // rows
    pad = torch.zeros(nb * rows - n, N, device="cuda", dtype=torch.float64)
    blocks = torch.cat([yv, pad]).view(nb, rows, N)
    cnt = torch.full((nb, 1), float(rows), device="cuda", dtype=torch.float64)
    cnt[-1] = n - (nb - 1) * rows
    sums = blocks.sum(1)
    mask = (torch.arange(rows, device="cuda")[None, :, None] < cnt[:, :, None]).double()
    m2 = (((blocks - (sums / cnt)[:, None, :]) * mask) ** 2).sum(1)
    assert rel_err(part[:nb, 0].cpu().numpy(), sums.cpu().numpy()) < 1e-5
    assert rel_err(part[:nb, 1].cpu().numpy(), m2.cpu().numpy()) < 1e-4
    # the BatchNorm that consumes them
    bn = torch.nn.BatchNorm1d(N, momentum=0.02).cuda()
    ref = torch.nn.BatchNorm1d(N, momentum=0.02).cuda()
    y._mvk_bn_stats = st
    out = ops.bn_lrelu(y, nv, bn, slope=0.1)
    want = torch.nn.functional.leaky_relu(ref(y[:n]), 0.1)
    assert (out[n:] == 0).all()
    assert rel_err(out[:n].detach().cpu().numpy(), want.detach().cpu().numpy()) < 2e-5
    assert rel_err(bn.running_mean.cpu().numpy(), ref.running_mean.cpu().numpy()) < 1e-5
    assert rel_err(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy()) < 1e-4


@pytest.mark.parametrize("M,N,K,split,n", [(19464, 64, 990, 4, 19000), (1300, 128, 1920, 6, 1300), (85, 512, 7680, 20, 85),
                                           (4096, 32, 480, 3, 4096), (333, 2048, 512, 2, 300), (19464, 32, 256, 2, 19464)])
def test_split_products_are_ordered_bit_reproducible_and_carry_statistics(ops, M, N, K, split, n):
    """The ordered split reduction (mvk_gemm_split_arena, csrc/gemm.hip): a product whose reduction is split over
    workgroups gives the SAME BITS on every run (the partial tiles are added in split order by the last-arriving
    workgroup, not with f32 atomics), needs no zero-initialised output (the output buffer is filled with NaN first),
    honours `accumulate`, and delivers the BatchNorm statistics of the complete sums. The counters it uses are back at
    zero afterwards (a second product on the same slices works)."""
    ops.set_deterministic(True)
    try:
        _split_products_ordered(ops, M, N, K, split, n)
    finally:
        ops.set_deterministic(False)


def _split_products_ordered(ops, M, N, K, split, n):
    assert ops.is_deterministic() and ops.lib().mvk_gemm_split_ordered() == 1
    torch.manual_seed(M + K)
    A = torch.randn(M, K, device="cuda")
    A[:, 0] = 7.0
    B = torch.randn(K, N, device="cuda")
    ref = (A.double() @ B.double())
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    outs = []
    for _ in range(6):
        y, st = ops.gemm(A, B, split_k=split, stats_n_valid=nv)
        outs.append((y.clone(), None if st is None else st[0].clone()))
    assert rel_err(outs[0][0].cpu().numpy(), ref.cpu().numpy()) < 1e-5
    for y, part in outs[1:]:
        assert torch.equal(y, outs[0][0])
        assert (part is None) == (outs[0][1] is None) and (part is None or torch.equal(part, outs[0][1]))
    sp, rows = ops.gemm_plan(M, N, K, split, True)
    assert sp == split
    if M > ops.bn_single_launch_rows(N):
        assert rows > 0 and outs[0][1] is not None          # statistics although the reduction is split
        part = outs[0][1]
        yv = outs[0][0][:n].double()
        nb = (n + rows - 1) // rows
        pad = torch.zeros(nb * rows - n, N, device="cuda", dtype=torch.float64)
        blocks = torch.cat([yv, pad]).view(nb, rows, N)
        assert rel_err(part[:nb, 0].cpu().numpy(), blocks.sum(1).cpu().numpy()) < 1e-5
    # a NaN-filled output is overwritten completely; accumulate adds the whole product once
    out = torch.full((M, N), float("nan"), device="cuda")
    ops.gemm(A, B, out=out, split_k=split)
    assert torch.equal(out, outs[0][0])
    base = torch.randn(M, N, device="cuda")
    acc = base.clone()
    ops.gemm(A, B, out=acc, accumulate=True, split_k=split)
    assert rel_err(acc.cpu().numpy(), (ref + base.double()).cpu().numpy()) < 1e-5
    # transposed operand layouts through the same epilogue
    yt = ops.gemm(A.t().contiguous(), B.t().contiguous(), transA=True, transB=True, split_k=split)
    assert rel_err(yt.cpu().numpy(), ref.cpu().numpy()) < 1e-5
    assert torch.equal(yt, ops.gemm(A.t().contiguous(), B.t().contiguous(), transA=True, transB=True, split_k=split))


def test_weight_gradients_of_a_backward_pass_are_bit_reproducible(ops):
    """The grouped weight-gradient launch (long reductions over the points, split many ways) with ordered splits: two
    backward passes over the same tensors give identical bits in every dW, in-line and deferred."""
    ops.set_deterministic(True)
    try:
        _weight_gradients_reproducible(ops)
    finally:
        ops.set_deterministic(False)


def _weight_gradients_reproducible(ops):
    torch.manual_seed(3)
    xs = [torch.randn(m, k, device="cuda") for m, k in ((19464, 64), (19464, 32), (4000, 128), (700, 990), (90, 1920))]
    gs = [torch.randn(x.shape[0], n, device="cuda") for x, n in zip(xs, (128, 64, 256, 64, 512))]
    runs = []
    for deferred in (False, True, True, False):
        Ws = [torch.nn.Parameter(torch.randn(g.shape[1], x.shape[1], device="cuda") * 0.05) for x, g in zip(xs, gs)]
        loss = sum((ops.linear(x, W) * g).sum() for x, W, g in zip(xs, Ws, gs))
        if deferred:
            with ops.defer_weight_grads():
                loss.backward()
        else:
            loss.backward()
        runs.append([W.grad.clone() for W in Ws])
    for i, (x, g) in enumerate(zip(xs, gs)):
        want = (g.double().t() @ x.double()).cpu().numpy()
        assert rel_err(runs[0][i].cpu().numpy(), want) < 1e-5 and rel_err(runs[1][i].cpu().numpy(), want) < 1e-5
        assert torch.equal(runs[0][i], runs[3][i]), i          # in-line twice
        assert torch.equal(runs[1][i], runs[2][i]), i          # grouped twice


@pytest.mark.parametrize("Nq,Ns,H,idt", [(3000, 3000, 40, torch.int32), (700, 2900, 33, torch.int64), (19464, 19464, 58, torch.int32),
                                         (50, 4000, 300, torch.int32),
                                         (2000, 60, 40, torch.int32)])          # rows of ~1000 entries: a workgroup per row
def test_reverse_neighbors_is_the_sorted_transposed_relation(ops, Nq, Ns, H, idt):
    """mvk_reverse_neighbors: row j of the result = the rows n of idx that contain j, ascending, padded with the shadow
    value -- against a NumPy transposition; the persistent counters are back at zero; a width that is too small raises the
    overflow word instead of passing silently; the sync-free form writes into a given matrix."""
    rng = np.random.default_rng(Nq + H)
    idx = np.stack([rng.choice(Ns + Ns // 3, size=H, replace=False) for _ in range(Nq)]).astype(np.int64)
    idx[idx >= Ns] = Ns                                  # a third of the entries are shadow entries
    idx[7] = Ns                                          # an all-shadow row
    want = [[] for _ in range(Ns)]
    for n in range(Nq):
        for j in idx[n]:
            if j < Ns:
                want[j].append(n)
    longest = max(len(r) for r in want)
    rev = ops.reverse_neighbors(T(idx).to(idt), Ns, sort=True)
    assert rev.dtype == torch.int32 and rev.shape == (Ns, max(longest, 1))
    unsorted = ops.reverse_neighbors(T(idx).to(idt), Ns, sort=False).cpu().numpy()        # order of arrival: same sets
    for j in range(0, Ns, max(1, Ns // 200)):
        assert sorted(unsorted[j, :len(want[j])]) == want[j] and (unsorted[j, len(want[j]):] == Nq).all(), j
    first = ops.reverse_neighbors(T(idx).to(idt), Ns, sort=True, first_column=True).cpu().numpy()   # idx[:, 0] alone
    col0 = idx[:, 0]
    for j in range(0, Ns, max(1, Ns // 200)):
        w = [n for n in np.nonzero(col0 == j)[0]]
        assert list(first[j, :len(w)]) == w and (first[j, len(w):] == Nq).all(), j
    got = rev.cpu().numpy()
    for j in range(0, Ns, max(1, Ns // 500)):
        assert list(got[j, :len(want[j])]) == want[j] and (got[j, len(want[j]):] == Nq).all(), j
    assert int(ops._rev_counts(Ns, torch.device("cuda:0"))[:Ns].abs().sum()) == 0
    # fixed width + status word, another shadow value, into a wider capacity matrix
    out = torch.full((Ns + 64, longest + 5), -7, dtype=torch.int32, device="cuda")
    st = torch.zeros(2, dtype=torch.int32, device="cuda")
    ops.reverse_neighbors(T(idx).to(idt), Ns, out=out, status=st, shadow=123456, sort=True)
    assert ops.check_reverse_status(st) == longest
    o = out.cpu().numpy()
    assert (o[Ns:] == -7).all()
    for j in range(0, Ns, max(1, Ns // 300)):
        assert list(o[j, :len(want[j])]) == want[j] and (o[j, len(want[j]):] == 123456).all(), j
    # the registry matches the tensor OBJECT, never a look-alike at another (or the same, recycled) address
    mat = T(idx).to(idt)
    ops.remember_reverse(mat, rev)
    assert ops.reverse_for(mat) is rev and ops.reverse_for(mat.clone()) is None and ops.reverse_for(mat, first_column=True) is None
    if longest > 2:
        st.zero_()
        ops.reverse_neighbors(T(idx).to(idt), Ns, width=longest - 1, status=st)
        with pytest.raises(RuntimeError, match="reverse neighbours"):
            ops.check_reverse_status(st)
        assert int(ops._rev_counts(Ns, torch.device("cuda:0"))[:Ns].abs().sum()) == 0


@pytest.mark.parametrize("M,K,Cin,Cout", [(19464, 15, 32, 32), (1300, 15, 128, 128), (85, 15, 512, 512), (700, 15, 66, 64), (33, 3, 5, 32)])
def test_kp_transposed_contraction_vs_float64(ops, M, K, Cin, Cout):
    """mvk_gemm_f32_kp_transposed: dx = sum_k A[:, k, :] . W[k]^T with the KPConv weights read in place (segmented B)."""
    torch.manual_seed(M)
    A = torch.randn(M, K, Cout, device="cuda")
    W = torch.randn(K, Cin, Cout, device="cuda") * 0.1
    want = torch.einsum("mko,kco->mc", A.double(), W.double()).cpu().numpy()
    assert rel_err(ops.kp_transposed_contraction(A, W).cpu().numpy(), want) < 1e-5


@pytest.mark.parametrize("Nq,Ns,H,C,strided", [(2500, 2500, 30, 32, False), (600, 2500, 28, 64, True), (19464, 19464, 45, 32, False),
                                               (90, 350, 20, 256, True)])
def test_kpconv_gather_form_feature_gradient(ops, Nq, Ns, H, C, strided):
    """The feature gradient of a rigid KPConv as a GATHER over the transposed neighbourhood relation (kpconv(..., rev=)):
    equal to the atomic scatter (same sums, another order: 1e-5) and to the float64 NumPy restatement (1e-4), and the
    same bits on every run; the weight gradient and the output are untouched."""
    from oracle import npref
    rng = np.random.default_rng(Nq + C)
    s = (rng.random((Ns, 3)) * 0.5).astype(np.float32)
    q = s.copy() if not strided else s[rng.choice(Ns, Nq, replace=False)] + rng.normal(0, 0.01, (Nq, 3)).astype(np.float32)
    d2 = ((q[:, None, :] - s[None, :, :]) ** 2).sum(-1) if Nq * Ns < 4e7 else None
    if d2 is not None:
        idx = np.argsort(d2, axis=1)[:, :H].astype(np.int32)
        idx[np.take_along_axis(d2, idx.astype(np.int64), 1) > 0.05 ** 2] = Ns           # radius crop -> shadow entries
    else:
        # (distinct entries per row, like every real neighbour matrix: a start plus increasing steps, modulo the range)
        idx = ((rng.integers(0, Ns + Ns // 4, (Nq, 1)) + np.cumsum(rng.integers(1, 7, (Nq, H)), 1)) % (Ns + Ns // 4)).astype(np.int32)
        idx[idx >= Ns] = Ns
    K = 15
    kp = (rng.normal(size=(K, 3)) * 0.02).astype(np.float32)
    x = rng.normal(size=(Ns, C)).astype(np.float32)
    W = (rng.normal(size=(K, C, C)) * 0.05).astype(np.float32)
    g = rng.normal(size=(Nq, C)).astype(np.float32)
    ops.set_deterministic(True)
    try:
        _gather_form_gradient(ops, q, s, idx, x, W, g, kp, Nq, Ns, H, C)
    finally:
        ops.set_deterministic(False)


def _gather_form_gradient(ops, q, s, idx, x, W, g, kp, Nq, Ns, H, C):
    from oracle import npref
    rev = ops.reverse_neighbors(T(idx), Ns)
    order = torch.randperm(Ns, device="cuda").to(torch.int32)
    res = []
    for use_rev in (False, True, True):
        xt, Wt = T(x).requires_grad_(True), T(W).requires_grad_(True)
        y, _ = ops.kpconv(T(q), T(s), T(idx), xt, T(kp), Wt, 0.03, rev=rev if use_rev else None,
                          rev_order=order if use_rev else None)
        (y * T(g)).sum().backward()
        res.append((y.detach(), xt.grad.clone(), Wt.grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    check_err("gather-form dx vs atomic scatter (Nq %d, C %d)" % (Nq, C), rel_err(res[1][1].cpu().numpy(), res[0][1].cpu().numpy()), 1e-5)
    assert torch.equal(res[1][1], res[2][1]), "gather-form dx differs between two runs"
    if Nq * H * C < 3e7:
        a64 = [q.astype(np.float64), s.astype(np.float64), idx.astype(np.int64), x.astype(np.float64), kp.astype(np.float64),
               W.astype(np.float64), 0.03]
        dx, dW = npref.kpconv_backward(*a64, g.astype(np.float64))
        check_err("gather-form dx vs float64 oracle (Nq %d, C %d)" % (Nq, C), rel_err(res[1][1].cpu().numpy(), dx), FP_TOL)
        assert rel_err(res[1][2].cpu().numpy(), dW) < FP_TOL


@pytest.mark.parametrize("Nq,Ns,H,C,strided", [(2500, 2500, 30, 32, False), (600, 2500, 28, 64, True), (19464, 19464, 45, 32, False)])
def test_kpconv_gather_form_feature_gradient_default_mode_arrival_order(ops, Nq, Ns, H, C, strided):
    """The same operator-level check in the DEFAULT mode: reverse lists whose rows are in order of
    ARRIVAL (no sort: what the bench and the input chain use), products with atomic split reductions. The feature
    gradient is held to the float64 NumPy restatement at the north_star tolerance and to the atomic scatter at 1e-5;
    it is NOT bit-identical between runs (the rows' order is not) -- only its distance from float64 is bounded."""
    from oracle import npref
    assert not ops.is_deterministic()
    rng = np.random.default_rng(Nq + C + 1)
    s = (rng.random((Ns, 3)) * 0.5).astype(np.float32)
    q = s.copy() if not strided else s[rng.choice(Ns, Nq, replace=False)] + rng.normal(0, 0.01, (Nq, 3)).astype(np.float32)
    if Nq * Ns < 4e7:
        d2 = ((q[:, None, :] - s[None, :, :]) ** 2).sum(-1)
        idx = np.argsort(d2, axis=1)[:, :H].astype(np.int32)
        idx[np.take_along_axis(d2, idx.astype(np.int64), 1) > 0.05 ** 2] = Ns
    else:
        idx = ((rng.integers(0, Ns + Ns // 4, (Nq, 1)) + np.cumsum(rng.integers(1, 7, (Nq, H)), 1)) % (Ns + Ns // 4)).astype(np.int32)
        idx[idx >= Ns] = Ns
    K = 15
    kp = (rng.normal(size=(K, 3)) * 0.02).astype(np.float32)
    x = rng.normal(size=(Ns, C)).astype(np.float32)
    W = (rng.normal(size=(K, C, C)) * 0.05).astype(np.float32)
    g = rng.normal(size=(Nq, C)).astype(np.float32)
    rev = ops.reverse_neighbors(T(idx), Ns, sort=False)                   # arrival order
    srt = ops.reverse_neighbors(T(idx), Ns, sort=True)
    assert torch.equal(torch.sort(rev, 1).values, torch.sort(srt, 1).values)
    res = []
    for r in (None, rev):
        xt, Wt = T(x).requires_grad_(True), T(W).requires_grad_(True)
        y, _ = ops.kpconv(T(q), T(s), T(idx), xt, T(kp), Wt, 0.03, rev=r)
        (y * T(g)).sum().backward()
        res.append((xt.grad.clone(), Wt.grad.clone()))
    check_err("default-mode gather-form dx vs atomic scatter (Nq %d, C %d)" % (Nq, C),
              rel_err(res[1][0].cpu().numpy(), res[0][0].cpu().numpy()), 1e-5)
    if Nq * H * C < 3e7:
        a64 = [q.astype(np.float64), s.astype(np.float64), idx.astype(np.int64), x.astype(np.float64), kp.astype(np.float64),
               W.astype(np.float64), 0.03]
        dx, dW = npref.kpconv_backward(*a64, g.astype(np.float64))
        check_err("default-mode gather-form dx vs float64 oracle (Nq %d, C %d)" % (Nq, C), rel_err(res[1][0].cpu().numpy(), dx), FP_TOL)
        check_err("default-mode dW vs float64 oracle (Nq %d, C %d)" % (Nq, C), rel_err(res[1][1].cpu().numpy(), dW), FP_TOL)


@pytest.mark.parametrize("b,n1,n2,transpose", [(2, 512, 1024, True), (3, 513, 1025, True), (3, 513, 1025, False), (3, 31, 63, True)])
def test_knn_replays_the_reference_knn_distance_test(ops, b, n1, n2, transpose):
    """mvpnet/ops/tests/test_knn_distance.py:37-54 replayed through the product's exact 3-NN (mvk_knn_f64): the reference
    test's shapes, layouts and seed (np.random.seed(0), randn queries / keys, k = 3), its expectation restated as in the
    test itself -- the full float32 distance matrix, torch.topk(largest=False, sorted=True) -- exact indices, distances
    to 1e-6. (The product searches in float64, the reference's CUDA op in float32: on these inputs no two candidates
    lie within float32 rounding of each other at the 3rd / 4th place, which the float64 brute force below confirms.)"""
    np.random.seed(0)
    k = 3
    if transpose:
        query_np = np.random.randn(b, 3, n1).astype(np.float32)
        key_np = np.random.randn(b, 3, n2).astype(np.float32)
        qs, ks = np.transpose(query_np, (0, 2, 1)), np.transpose(key_np, (0, 2, 1))
    else:
        query_np = np.random.randn(b, n1, 3).astype(np.float32)
        key_np = np.random.randn(b, n2, 3).astype(np.float32)
        qs, ks = query_np, key_np
    for i in range(b):
        q, kk = torch.from_numpy(np.ascontiguousarray(qs[i])).cuda(), torch.from_numpy(np.ascontiguousarray(ks[i])).cuda()
        # the reference test's expectation (bpdist2 + topk, float32)
        dist = ((q.unsqueeze(1) - kk.unsqueeze(0)) ** 2).sum(2)
        d_want, i_want = torch.topk(dist, k, dim=1, largest=False, sorted=True)
        got = ops.knn_pixels(q, kk.double().view(1, n2, 1, 3), torch.ones((1, n2, 1), dtype=torch.bool, device="cuda"), k=k)
        d64 = ((qs[i].astype(np.float64)[:, None, :] - ks[i].astype(np.float64)[None, :, :]) ** 2).sum(2)
        exact = np.argsort(d64, axis=1, kind="stable")[:, :k]
        assert np.array_equal(got.cpu().numpy(), exact)
        np.testing.assert_equal(got.cpu().numpy(), i_want.cpu().numpy())
        d_got = torch.gather(dist, 1, got)
        np.testing.assert_allclose(d_got.cpu().numpy(), d_want.cpu().numpy(), atol=1e-6)


def test_deferred_weight_gradients_run_as_one_grouped_launch(ops):
    """ops.defer_weight_grads(): the dW products recorded during a backward pass (TN, wide and narrow outputs, ragged
    sizes, split and unsplit reductions) come out of the grouped launch equal to the individual products; under
    hipGraph capture too (table copy = a memcpy node)."""
    torch.manual_seed(5)
    shapes = [(19464, 990, 64), (3986, 960, 64), (65, 7680, 512), (19464, 64, 32), (19464, 128, 20), (300, 70, 45), (1, 33, 17),
              (5000, 30, 64), (19464, 32, 128)]
    As = [torch.randn(k, m, device="cuda") for (k, m, n) in shapes]
    Bs = [torch.randn(k, n, device="cuda") for (k, m, n) in shapes]
    want = [(a.double().t() @ b.double()).cpu().numpy() for a, b in zip(As, Bs)]
    with ops.defer_weight_grads():
        outs = [ops._dw_gemm(a, b) for a, b in zip(As, Bs)]
        small = ops._dw_gemm(As[0][:, :8], Bs[0][:, :9])            # N <= 16: not grouped, computed at once
    for o, w in zip(outs, want):
        assert rel_err(o.cpu().numpy(), w) < 1e-5
    assert rel_err(small.cpu().numpy(), (As[0][:, :8].double().t() @ Bs[0][:, :9].double()).cpu().numpy()) < 1e-5
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            with ops.defer_weight_grads():
                cap = [ops._dw_gemm(a, b) for a, b in zip(As[1:4], Bs[1:4])]
        for o in cap:
            o.zero_()
        g.replay()
        torch.cuda.synchronize()
    for o, w in zip(cap, want[1:4]):
        assert rel_err(o.cpu().numpy(), w) < 1e-5


def test_deferred_weight_gradients_with_existing_grads_and_shared_weights(ops):
    """ADVICE r2 (ops.defer_weight_grads hazard): a parameter that already holds a .grad (zero_grad(set_to_none=False),
    micro-batch accumulation, a second backward stage through the same weight) must ACCUMULATE correctly -- its product
    runs in line instead of being deferred; a weight used twice inside one scope is refused loudly; a deferred result
    that autograd consumed instead of adopting (a hook that copies the gradient) raises at the flush instead of losing
    the product silently."""
    torch.manual_seed(11)
    x = torch.randn(3000, 96, device="cuda")
    W = torch.nn.Parameter(torch.randn(64, 96, device="cuda") * 0.1)
    want = (torch.ones(3000, 64, device="cuda").double().t() @ x.double())

    def backward_once():
        with ops.defer_weight_grads():
            ops.linear(x, W).sum().backward()

    backward_once()                                         # .grad is None: deferred, adopted
    assert rel_err(W.grad.cpu().numpy(), want.cpu().numpy()) < 1e-5
    backward_once()                                         # .grad exists: in line, accumulated
    backward_once()
    assert rel_err(W.grad.cpu().numpy(), (3 * want).cpu().numpy()) < 1e-5
    W.grad = None
    with pytest.raises(RuntimeError, match="two weight gradients"):
        with ops.defer_weight_grads():
            (ops.linear(x, W).sum() + ops.linear(2 * x, W).sum()).backward()
    W.grad = None
    # the same through a KPConv layer (the weight is input 5 of the node)
    q = torch.rand(500, 3, device="cuda")
    idx = torch.randint(0, 501, (500, 12), device="cuda", dtype=torch.int32)
    feats = torch.randn(500, 32, device="cuda")
    kp = (torch.rand(15, 3, device="cuda") - 0.5) * 0.2
    Wk = torch.nn.Parameter(torch.randn(15, 32, 48, device="cuda") * 0.1)

    def kp_backward():
        with ops.defer_weight_grads():
            ops.kpconv(q, q, idx, feats, kp, Wk, 0.12)[0].sum().backward()

    kp_backward()
    g1 = Wk.grad.clone()
    kp_backward()
    assert rel_err(Wk.grad.cpu().numpy(), (2 * g1).cpu().numpy()) < 1e-5
    # a non-leaf weight whose gradient is consumed (not adopted) before the flush: loud
    Wn = torch.nn.Parameter(torch.randn(64, 96, device="cuda") * 0.1)
    with pytest.raises(RuntimeError, match="consumed before the grouped launch"):
        with ops.defer_weight_grads():
            ops.linear(x, Wn * 2.0).sum().backward()         # MulBackward reads dW at once and drops it


@pytest.mark.parametrize("R,C,slope", [(19464, 128, 0.1), (19464, 20, 0.1), (300, 1, 0.1), (5000, 256, 1.0), (1, 7, 0.1)])
def test_bias_lrelu_vs_torch(ops, R, C, slope):
    """The BatchNorm-less form of BatchNormBlock + LeakyReLU (blocks.py:462-463, the two head layers) in one launch each
    way: output and input gradient bit for bit (same single operations), bias gradient = column sums to 1e-5."""
    torch.manual_seed(R + C)
    x = torch.randn(R, C, device="cuda", requires_grad=True)
    b = torch.randn(C, device="cuda", requires_grad=True)
    g = torch.randn(R, C, device="cuda")
    y = ops.bias_lrelu(x, b, slope)
    gx, gb = torch.autograd.grad(y, [x, b], g)
    xr, br = x.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = torch.nn.functional.leaky_relu(xr + br, slope)
    gxr, gbr = torch.autograd.grad(yr, [xr, br], g)
    assert torch.equal(y, yr) and torch.equal(gx, gxr)
    assert rel_err(gb.cpu().numpy(), gbr.cpu().numpy()) < 1e-5


@pytest.mark.parametrize("M,Kd,N", [(19464, 128, 32), (4986, 256, 64), (330, 1024, 256), (85, 2048, 512), (1, 16, 8)])
def test_linear_passthrough_sums_the_two_gradients_inside_the_gemm(ops, M, Kd, N):
    """ops.linear(..., passthrough=True): y = x W^T and an alias x' of x for a second consumer (the shortcut of a
    residual block, blocks.py:638-649); the backward adds g W onto the second consumer's gradient inside the GEMM
    (split or unsplit plans) -- the input gradient must equal autograd's sum of the two, the weight gradient is
    untouched, and an unused alias costs nothing."""
    torch.manual_seed(M + Kd)
    x = torch.randn(M, Kd, device="cuda", requires_grad=True)
    W = (torch.randn(N, Kd, device="cuda") * 0.1).requires_grad_(True)
    gy, gs = torch.randn(M, N, device="cuda"), torch.randn(M, Kd, device="cuda")
    y, xs = ops.linear(x, W, passthrough=True)
    gx, gW = torch.autograd.grad([y, xs * 1.5], [x, W], [gy, gs])
    want_x = gy.double() @ W.detach().double() + 1.5 * gs.double()
    want_W = gy.double().t() @ x.detach().double()
    assert rel_err(gx.cpu().numpy(), want_x.cpu().numpy()) < 1e-5 and rel_err(gW.cpu().numpy(), want_W.cpu().numpy()) < 1e-5
    y2, xs2 = ops.linear(x, W, passthrough=True)            # alias unused: plain product
    (gx2,) = torch.autograd.grad(y2, x, gy)
    assert rel_err(gx2.cpu().numpy(), (gy.double() @ W.detach().double()).cpu().numpy()) < 1e-5
    y3, xs3 = ops.linear(x, W, passthrough=True)            # only the alias used: its gradient passes through
    (gx3,) = torch.autograd.grad(xs3, x, gs)
    assert torch.equal(gx3, gs)


# ------------------------------------------------------------------ masked BatchNorm + LeakyReLU

@pytest.mark.parametrize("slope", [1.0, 0.1])
@pytest.mark.parametrize("R,D,n", [(50, 64, 50), (128, 32, 100), (3000, 128, 2873), (19464, 64, 19464),
                                   (19464, 66, 19000), (40000, 32, 40000), (4096, 200, 4000),
                                   (129, 64, 129), (923, 128, 900), (1024, 512, 1024), (225, 256, 2), (600, 36, 577),
                                   (700, 66, 700)])
def test_masked_bn_lrelu_vs_torch(ops, R, D, n, slope):
    """blocks.py:430-467 + LeakyReLU: the single-workgroup (R <= 128) and the three-launch kernels against
    torch's batch_norm on the valid rows (129..1024 rows with D % 4 == 0: the vectorised single-launch kernels);
    padded rows come back as zeros, running statistics and the batch
    counter move like nn.BatchNorm1d's. slope = 1 checks every gradient tightly; with slope = 0.1 a
    last-bit difference of the normalised value flips the slope of elements sitting on the kink, so the
    input gradient is compared away from it and the parameter gradients (sums over all rows) loosely."""
    torch.manual_seed(R + D)
    x = (torch.randn(R, D, device="cuda") * 2 + 3).requires_grad_(True)
    bn = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    ref.load_state_dict(bn.state_dict())
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    go = torch.randn(R, D, device="cuda")
    for _ in range(2):
        y = ops.bn_lrelu(x, nv, bn, slope=slope)
        gx, gw, gb = torch.autograd.grad(y, [x, bn.weight, bn.bias], go)
    xr = x.detach()[:n].clone().requires_grad_(True)
    for _ in range(2):
        yr = torch.nn.functional.leaky_relu(ref(xr), slope)
        gxr, gwr, gbr = torch.autograd.grad(yr, [xr, ref.weight, ref.bias], go[:n])
    assert (y[n:] == 0).all() and (gx[n:] == 0).all()
    assert rel_err(y[:n].detach().cpu().numpy(), yr.detach().cpu().numpy()) < 1e-5
    away = (yr.detach().abs() > 1e-4).float() if slope != 1.0 else torch.ones_like(yr)
    assert away.mean() > 0.99
    ptol = 1e-4 if slope == 1.0 else 1e-2
    assert rel_err((gx[:n] * away).cpu().numpy(), (gxr * away).cpu().numpy()) < ptol
    assert rel_err(gw.cpu().numpy(), gwr.cpu().numpy()) < ptol and rel_err(gb.cpu().numpy(), gbr.cpu().numpy()) < ptol
    assert rel_err(bn.running_mean.cpu().numpy(), ref.running_mean.cpu().numpy()) < 1e-5
    assert rel_err(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy()) < 1e-5
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2


@pytest.mark.parametrize("M,N,Kd", [(19464, 64, 990), (19464, 32, 480), (4986, 64, 960), (4100, 64, 30), (40000, 32, 150),
                                    (55070, 64, 1024), (5000, 32, 16), (100003, 64, 990)])
def test_gemm_f32_stream(ops, M, N, Kd, monkeypatch):
    """The streaming f32 contraction of the big rigid layers (csrc/gemm32s.hip; reference shape contract
    models/blocks.py:370-374): equals the float64 product to f32 summation order (2e-6 of the largest output), equals
    the tiled kernel's result to the same bound, statistics partials against NumPy, two launches bit-identical (no
    atomics), NaN-filled slack behind A harmless (the surplus columns are masked, not multiplied by zero)."""
    torch.manual_seed(M + N + Kd)
    # the default plan takes the kernel only where it measured faster than the tiled one (N = 64, Kd > 512, M >= 98 304);
    # MVK_GEMM32_STREAM=2 (read per call) opens every supported shape to it for this test
    assert ops.gemm_f32_stream_plan(M, N, Kd)[0] == (M >= 98304 and N == 64 and Kd > 512)
    monkeypatch.setenv("MVK_GEMM32_STREAM", "2")
    ok, tiles, wgs, need = ops.gemm_f32_stream_plan(M, N, Kd)
    assert ok and need == 0
    buf = torch.full((M * Kd + 64,), float("nan"), device="cuda")
    A = buf[:M * Kd].view(M, Kd)
    A.copy_(torch.randn(M, Kd, device="cuda"))
    W = torch.randn(Kd, N, device="cuda") * 0.2
    want = A.double() @ W.double()
    scale = want.abs().max().item()
    y, st = ops.gemm_f32_stream(A, W)
    assert st is None and torch.isfinite(y).all()
    assert (y.double() - want).abs().max().item() / scale < 2e-6
    assert (y - ops.gemm(A, W)).abs().max().item() / scale < 2e-6
    nv = M - 37
    n_valid = torch.tensor([nv], dtype=torch.int32, device="cuda")
    y2, (part, rows) = ops.gemm_f32_stream(A, W, n_valid)
    assert torch.equal(y, y2) and rows == 16 * tiles and part.shape == (wgs, 2, N)
    yv = y.double().cpu().numpy()
    for b in sorted({0, wgs // 2, wgs - 1}):
        blk = yv[b * rows:min((b + 1) * rows, nv)]
        got_sum, got_m2 = part[b, 0].double().cpu().numpy(), part[b, 1].double().cpu().numpy()
        if blk.shape[0] == 0:
            assert (got_sum == 0).all() and (got_m2 == 0).all()
            continue
        assert np.abs(got_sum - blk.sum(0)).max() < 1e-5 * max(np.abs(blk).sum(0).max(), 1e-30)
        m2_ref = ((blk - blk.mean(0)) ** 2).sum(0)
        assert np.abs(got_m2 - m2_ref).max() < 1e-4 * max(m2_ref.max(), 1e-30) + 1e-30
    bn, ref = torch.nn.BatchNorm1d(N, momentum=0.02).cuda(), torch.nn.BatchNorm1d(N, momentum=0.02).cuda()
    y2._mvk_bn_stats = (part, rows)
    out = ops.bn_lrelu(y2, n_valid, bn, slope=0.1)
    outr = torch.nn.functional.leaky_relu(ref(y[:nv]), 0.1)
    assert rel_err(out[:nv].detach().cpu().numpy(), outr.detach().cpu().numpy()) < 2e-5 and (out[nv:] == 0).all()
    # shapes no plan gives to the streaming kernel
    for (m, n, k) in ((3000, 64, 990), (19464, 128, 1920), (19464, 64, 75), (19464, 64, 1100), (19464, 48, 480)):
        assert not ops.gemm_f32_stream_plan(m, n, k)[0]


@pytest.mark.parametrize("R,D,n", [(100, 64, 90), (3000, 128, 2873), (19464, 64, 19464), (4096, 200, 4000),
                                   (923, 128, 900), (225, 512, 225)])
def test_masked_bn_with_residual_join_vs_torch(ops, R, D, n):
    """y = LeakyReLU(BN(x) + shortcut) in one launch (ResnetBottleneckBlock's join, blocks.py:644-649) against
    the unfused torch expression: output, and the gradients of x, the shortcut and the BN parameters."""
    torch.manual_seed(R * 3 + D)
    x = (torch.randn(R, D, device="cuda") * 2 + 1).requires_grad_(True)
    sc = torch.randn(R, D, device="cuda").requires_grad_(True)
    bn = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    ref.load_state_dict(bn.state_dict())
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    go = torch.randn(R, D, device="cuda")
    y = ops.bn_lrelu(x, nv, bn, slope=0.1, addend=sc)
    gx, gs, gw, gb = torch.autograd.grad(y, [x, sc, bn.weight, bn.bias], go)
    xr, sr = x.detach()[:n].clone().requires_grad_(True), sc.detach()[:n].clone().requires_grad_(True)
    yr = torch.nn.functional.leaky_relu(ref(xr) + sr, 0.1)
    gxr, gsr, gwr, gbr = torch.autograd.grad(yr, [xr, sr, ref.weight, ref.bias], go[:n])
    assert (y[n:] == 0).all() and (gx[n:] == 0).all() and (gs[n:] == 0).all()
    assert rel_err(y[:n].detach().cpu().numpy(), yr.detach().cpu().numpy()) < 1e-5
    away = (yr.detach().abs() > 1e-4).float()                      # elements on the LeakyReLU kink may flip slope
    assert away.mean() > 0.99
    assert rel_err((gs[:n] * away).cpu().numpy(), (gsr * away).cpu().numpy()) < 1e-6
    assert rel_err((gx[:n] * away).cpu().numpy(), (gxr * away).cpu().numpy()) < 1e-2
    assert rel_err(gw.cpu().numpy(), gwr.cpu().numpy()) < 1e-2 and rel_err(gb.cpu().numpy(), gbr.cpu().numpy()) < 1e-2


@pytest.mark.parametrize("slope", [1.0, 0.1])
@pytest.mark.parametrize("join", [False, True])
def test_masked_bn_misaligned_base_takes_two_stage_kernels_vs_torch(ops, join, slope):
    """300 rows x 64 channels is the register-resident family's shape, but input, shortcut and upstream gradient start
    one float past a 16-byte boundary: the float4 kernels must not run, the two-stage ones do. Against torch under the
    bounds of test_masked_bn_lrelu_vs_torch (the shortcut's gradient: the 1e-6 of the residual-join test)."""
    R, D, n = 300, 64, 263
    torch.manual_seed(R + D)
    x = off_by_one_float(torch.randn(R, D, device="cuda") * 2 + 3).requires_grad_(True)
    sc = off_by_one_float(torch.randn(R, D, device="cuda")).requires_grad_(True) if join else None
    go = off_by_one_float(torch.randn(R, D, device="cuda"))
    bn = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    with torch.no_grad():
        bn.weight.uniform_(0.5, 1.5)
        bn.bias.uniform_(-0.5, 0.5)
    ref = torch.nn.BatchNorm1d(D, momentum=0.02).cuda()
    ref.load_state_dict(bn.state_dict())
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    leaves = [x, bn.weight, bn.bias] + ([sc] if join else [])
    for _ in range(2):
        y = ops.bn_lrelu(x, nv, bn, slope=slope, addend=sc)
        gx, gw, gb, *gs = torch.autograd.grad(y, leaves, go)
    xr = x.detach()[:n].clone().requires_grad_(True)
    sr = sc.detach()[:n].clone().requires_grad_(True) if join else None
    for _ in range(2):
        yr = torch.nn.functional.leaky_relu(ref(xr) + sr if join else ref(xr), slope)
        gxr, gwr, gbr, *gsr = torch.autograd.grad(yr, [xr, ref.weight, ref.bias] + ([sr] if join else []), go[:n])
    assert (y[n:] == 0).all() and (gx[n:] == 0).all()
    assert rel_err(y[:n].detach().cpu().numpy(), yr.detach().cpu().numpy()) < 1e-5
    away = (yr.detach().abs() > 1e-4).float() if slope != 1.0 else torch.ones_like(yr)
    assert away.mean() > 0.99
    ptol = 1e-4 if slope == 1.0 else 1e-2
    assert rel_err((gx[:n] * away).cpu().numpy(), (gxr * away).cpu().numpy()) < ptol
    assert rel_err(gw.cpu().numpy(), gwr.cpu().numpy()) < ptol and rel_err(gb.cpu().numpy(), gbr.cpu().numpy()) < ptol
    if join:
        assert (gs[0][n:] == 0).all()
        assert rel_err((gs[0][:n] * away).cpu().numpy(), (gsr[0] * away).cpu().numpy()) < 1e-6
    assert rel_err(bn.running_mean.cpu().numpy(), ref.running_mean.cpu().numpy()) < 1e-5
    assert rel_err(bn.running_var.cpu().numpy(), ref.running_var.cpu().numpy()) < 1e-5
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2


# ------------------------------------------------------------------ fused clip + SGD

def test_fused_clip_sgd_matches_torch_clip_and_sgd():
    """mvk_sgd_clip_step against torch.nn.utils.clip_grad_value_ + torch.optim.SGD (momentum, weight decay, two
    parameter groups with their own learning rate, utils/trainer.py:72-79, 190-195) over several steps, tensors
    of awkward sizes (1 element, not a multiple of 4, larger than one chunk), one parameter without a gradient."""
    import mvkpconv
    optim = mvkpconv.sub("optim")
    torch.manual_seed(0)
    shapes = [(1,), (7,), (64,), (15, 66, 64), (4097,), (3, 5), (20000, 3), (33,)]
    ours = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    mine = optim.FusedClipSGD([{"params": ours[:5]}, {"params": ours[5:], "lr": 1e-3}], lr=1e-2, momentum=0.98,
                              weight_decay=1e-3, clip_value=0.5)
    theirs = torch.optim.SGD([{"params": ref[:5]}, {"params": ref[5:], "lr": 1e-3}], lr=1e-2, momentum=0.98,
                             weight_decay=1e-3)
    for step in range(4):
        for a, b in zip(ours, ref):
            g = torch.randn_like(a) * (1.0 if step % 2 else 0.3)
            a.grad, b.grad = g.clone(), g.clone()
        ours[6].grad = None if step == 2 else ours[6].grad          # a parameter that got no gradient this step
        ref[6].grad = None if step == 2 else ref[6].grad
        torch.nn.utils.clip_grad_value_(ref, 0.5)
        theirs.step()
        mine.step()
        for a, b in zip(ours, ref):
            assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-6
    for a, b in zip(ours, ref):
        if b in theirs.state and "momentum_buffer" in theirs.state[b]:
            assert rel_err(mine.state[a]["momentum_buffer"].cpu().numpy(), theirs.state[b]["momentum_buffer"].cpu().numpy()) < 1e-6
    # under hipGraph capture (fixed gradient addresses, the table copy becomes a memcpy node)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for a in ours:
            a.grad = torch.zeros_like(a)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            mine.step()
        for rep in range(2):                 # nothing ran during the capture: two replays = two more steps
            for a, b in zip(ours, ref):
                a.grad.copy_(torch.full_like(a, 0.7 - rep))
                b.grad = torch.full_like(b, 0.7 - rep)
            g.replay()
            torch.nn.utils.clip_grad_value_(ref, 0.5)
            theirs.step()
        torch.cuda.synchronize()
    for a, b in zip(ours, ref):
        assert rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-6


def test_fused_clip_sgd_trainer_contract():
    """what the reference's trainer asks of its optimiser beyond step() -- (1) grad_clip_norm <= 0 means no
    clipping (trainer.py:191), (2) state_dict() / load_state_dict() in torch.optim.SGD's layout, interchangeable with a
    torch SGD over the same parameters (trainer.py:101, 251), (3) the per-epoch learning-rate decay written into
    param_groups (trainer.py:239-241) reaches the CAPTURED step after sync_hyperparameters(), (4) an eager step after a
    capture does not run on the captured table."""
    import mvkpconv
    optim = mvkpconv.sub("optim")
    torch.manual_seed(3)
    shapes = [(5,), (300, 7), (4100,)]
    ours = [torch.nn.Parameter(torch.randn(s, device="cuda")) for s in shapes]
    ref = [torch.nn.Parameter(p.detach().clone()) for p in ours]
    mine = optim.FusedClipSGD([{"params": ours[:2]}, {"params": ours[2:], "lr": 1e-3}], lr=1e-2, momentum=0.9,
                              weight_decay=1e-3, clip_value=0.0)                       # (1) no clipping
    theirs = torch.optim.SGD([{"params": ref[:2]}, {"params": ref[2:], "lr": 1e-3}], lr=1e-2, momentum=0.9, weight_decay=1e-3)

    def same():
        return all(rel_err(a.detach().cpu().numpy(), b.detach().cpu().numpy()) < 1e-6 for a, b in zip(ours, ref))

    for _ in range(2):
        for a, b in zip(ours, ref):
            g = torch.randn_like(a) * 5
            a.grad, b.grad = g.clone(), g.clone()
        mine.step()
        theirs.step()
    assert same()
    # (2) our state into a fresh torch SGD, torch's state into a fresh FusedClipSGD: both continue identically
    sd = mine.state_dict()
    assert set(sd) == {"state", "param_groups"} and sd["param_groups"][1]["lr"] == 1e-3 and sd["param_groups"][0]["params"] == [0, 1]
    theirs2 = torch.optim.SGD([{"params": ref[:2]}, {"params": ref[2:], "lr": 5.0}], lr=5.0, momentum=0.1)
    theirs2.load_state_dict(sd)
    mine2 = optim.FusedClipSGD([{"params": ours[:2]}, {"params": ours[2:]}], lr=7.0, momentum=0.0, clip_value=-1.0)
    mine2.load_state_dict(theirs.state_dict())
    assert mine2.momentum == 0.9 and mine2.param_groups[1]["lr"] == 1e-3 and mine2.param_groups[0]["weight_decay"] == 1e-3
    for a, b in zip(ours, ref):
        g = torch.randn_like(a)
        a.grad, b.grad = g.clone(), g.clone()
    mine2.step()
    theirs2.step()
    assert same()
    # (3) + (4): capture a step, decay the rates in place like the trainer, replay
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        for a in ours:
            a.grad = torch.zeros_like(a)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=st):
            mine2.step()
        for rep in range(3):
            if rep == 1:
                for g1, g2 in zip(mine2.param_groups, theirs2.param_groups):
                    g1["lr"] *= 0.5
                    g2["lr"] *= 0.5
                assert mine2.sync_hyperparameters() == 1
            for a, b in zip(ours, ref):
                a.grad.copy_(torch.full_like(a, 0.3 + rep))
                b.grad = torch.full_like(b, 0.3 + rep)
            graph.replay()
            theirs2.step()
        torch.cuda.synchronize()
        assert same()
        for a, b in zip(ours, ref):                   # eager step with the SAME tensors right after the capture
            b.grad = a.grad.clone()
        mine2.step()
        theirs2.step()
        torch.cuda.synchronize()
    assert same()


# ------------------------------------------------------------------ deformable: regulariser kernel

def regulariser_float64(min_d2, dkp, n, ext, rep, power):
    """The cited lines of p2p_fitting_regularizer (models/architectures.py:20-58) for ONE layer with tensor ops in float64
    over the first n rows: (loss term, min_d2[:n] leaf, deformed_KP[:n] leaf) -- differentiate the first wrt the others."""
    K = min_d2.shape[1]
    m64 = min_d2.detach().double()[:n].requires_grad_(True)
    k64 = dkp.detach().double()[:n].requires_grad_(True)
    l1 = torch.nn.L1Loss()
    fit = l1(m64 / ext ** 2, torch.zeros_like(m64))
    locs = k64 / ext
    rl = 0
    for i in range(K):
        other = torch.cat([locs[:, :i, :], locs[:, i + 1:, :]], dim=1).detach()
        d = torch.sqrt(torch.sum((other - locs[:, i:i + 1, :]) ** 2, dim=2))
        r = torch.sum(torch.clamp_max(d - rep, max=0.0) ** 2, dim=1)
        rl = rl + l1(r, torch.zeros_like(r)) / K
    return power * (2 * fit + rl), m64, k64


@pytest.mark.parametrize("N,n", [(300, 300), (2000, 1873), (1, 1)])
def test_deform_regularizer_kernel_vs_reference_formula(ops, N, n):
    """mvk_deform_regularizer against the cited lines of p2p_fitting_regularizer (models/architectures.py:20-58)
    written with tensor ops in float64: the layer's loss term and the gradients wrt min_d2 and deformed_KP, with a
    row count below the capacity (padded rows must not contribute and must get zero gradient)."""
    torch.manual_seed(N)
    K, ext, rep, power = 15, 0.6, 1.2, 1.0
    min_d2 = (torch.rand(N, K, device="cuda") * 0.3).requires_grad_(True)
    dkp = (torch.randn(N, K, 3, device="cuda") * 0.4).requires_grad_(True)
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    loss = ops.deform_regularizer(min_d2, dkp, ext, rep, power, nv)
    g1, g2 = torch.autograd.grad(loss, [min_d2, dkp])
    want, m64, k64 = regulariser_float64(min_d2, dkp, n, ext, rep, power)
    w1, w2 = torch.autograd.grad(want, [m64, k64])
    assert abs(loss.item() - want.item()) < 1e-5 * abs(want.item())
    assert rel_err(g1[:n].cpu().numpy(), w1.cpu().numpy()) < 1e-5 and rel_err(g2[:n].cpu().numpy(), w2.cpu().numpy()) < 1e-5
    assert (g1[n:] == 0).all() and (g2[n:] == 0).all()


# ------------------------------------------------------------------ frozen 2D encoder fast path

@pytest.mark.parametrize("hw", [(120, 160), (60, 80)])
def test_frozen_encoder_fast_path_equals_the_module_forward(hw):
    """UNetResNet34 in eval mode with frozen weights: BatchNorm folded into the convolutions + the fused pointwise
    epilogue (ops.bias_act_nhwc, channels-last) against the module-by-module forward (non-trivial running
    statistics, ragged padding to a multiple of 16)."""
    import mvkpconv
    unet = importlib.import_module(mvkpconv.PKG_NAME + ".dropin.mvpnet.models.unet_resnet34")
    torch.manual_seed(3)
    net = unet.UNetResNet34(20, p=0.5).cuda()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.running_mean.normal_(0, 0.2)
                m.running_var.uniform_(0.5, 1.5)
                m.weight.uniform_(0.5, 1.5)
                m.bias.normal_(0, 0.2)
    for p in net.parameters():
        p.requires_grad = False
    net.eval()
    x = torch.randn(3, 3, hw[0], hw[1], device="cuda")
    assert net._frozen_ok(x)
    with torch.no_grad():
        want = net._forward_modules(x)["feature"]
        got = net({"image": x})["feature"]
    assert got.shape == want.shape == (3, 64, hw[0], hw[1])
    assert rel_err(got.cpu().numpy(), want.cpu().numpy()) < 2e-4        # MIOpen picks its algorithm per layout / shape
    net.train()
    assert not net._frozen_ok(x)


# ------------------------------------------------------------------ group_points (reference test shapes)

def test_group_points_float64_like_the_reference_extension(ops):
    """group_points_kernel.cu:60,130 dispatch float and double: the double path, forward and backward."""
    torch.manual_seed(1)
    pts = torch.randn(2, 5, 300, dtype=torch.float64).cuda().requires_grad_(True)
    index = torch.randint(0, 300, [2, 77, 9]).long().cuda()
    want = pts.unsqueeze(2).expand(2, 5, 77, 300).gather(3, index.unsqueeze(1).expand(2, 5, 77, 9))
    got = ops.group_points(pts, index)
    assert got.dtype == torch.float64 and torch.equal(got, want)
    go = torch.randn_like(want)
    gw, = torch.autograd.grad(want, pts, go, retain_graph=True)
    gg, = torch.autograd.grad(got, pts, go)
    assert torch.allclose(gg, gw, rtol=1e-12, atol=1e-12)


@pytest.mark.parametrize("b,c,n1,n2,k", [(2, 3, 512, 128, 32), (5, 64, 513, 129, 33)])
def test_group_points_reference_test_shapes(ops, b, c, n1, n2, k):
    """Same shapes / seed / restatement as mvpnet/ops/tests/test_group_points.py:6-44."""
    torch.manual_seed(0)
    pts = torch.randn(b, c, n1).cuda().requires_grad_(True)
    index = torch.randint(0, n1, [b, n2, k]).long().cuda()
    want = pts.unsqueeze(2).expand(b, c, n2, n1).gather(3, index.unsqueeze(1).expand(b, c, n2, k))
    got = ops.group_points(pts, index)
    assert torch.allclose(got, want)
    go = torch.randn_like(want)
    gw, = torch.autograd.grad(want, pts, go, retain_graph=True)
    gg, = torch.autograd.grad(got, pts, go)
    assert torch.allclose(gg, gw, atol=1e-5)


# ------------------------------------------------------------------ edge cases / error paths

def _knn_scene(seed, nq, nk_side):
    """Three overlapping 'depth maps' of a wall + floor (row-major pixel order), queries on and far off
    the surfaces, duplicated keys (exact ties), invalid pixels, keys beyond the 3.2 m torus period."""
    rng = np.random.default_rng(seed)
    u, v = np.meshgrid(np.linspace(-1.5, 1.5, nk_side), np.linspace(0, 2.2, nk_side))
    wall = np.stack([u.ravel(), np.full(u.size, 1.3), v.ravel()], 1)
    floor = np.stack([u.ravel(), v.ravel() - 0.9, np.zeros(u.size)], 1)
    far = np.stack([u.ravel() * 3, v.ravel() * 2 + 3.0, np.full(u.size, 0.4)], 1)
    keys = np.concatenate([wall, floor, far], 0) + rng.normal(0, 0.004, (3 * u.size, 3))
    keys[100:200] = keys[300:400]                          # exact duplicates -> (d2, index) tie rule
    valid = rng.random(keys.shape[0]) > 0.1
    q = np.concatenate([keys[rng.integers(0, keys.shape[0], nq // 2)] + rng.normal(0, 0.02, (nq // 2, 3)),
                        rng.uniform(-1.2, 1.2, (nq - nq // 2, 3)) + [0, 0, 1.0]], 0).astype(np.float32)
    q[:50] = keys[100:150].astype(np.float32)              # queries sitting on the duplicated keys
    return q, keys, valid


@pytest.mark.parametrize("k", [3, 1, 5])
def test_knn_pruned_vs_oracle_and_brute_force(ops, k, monkeypatch):
    """The box-pruned 3-NN (taken for nq >= 1024, nk >= 4096) returns exactly what the brute-force
    kernels and the CPU oracle return (ScanNet_sphere_color.py:448-451 contract: exact, float64)."""
    from oracle import cport
    q, keys, valid = _knn_scene(3, 3000, 70)               # 3000 x 14700
    shape = (3, 70, 70)
    Tq, Tk, Tv = T(q), T(keys.reshape(shape + (3,))), T(valid.reshape(shape))
    got = ops.knn_pixels(Tq, Tk, Tv, k=k).cpu().numpy()
    ind_all = np.nonzero(valid)[0]
    want = ind_all[cport.knn_f64(q.astype(np.float64), keys[ind_all], k)[0]]
    assert np.array_equal(got, want)
    monkeypatch.setenv("MVK_KNN_BRUTE", "1")
    assert np.array_equal(ops.knn_pixels(Tq, Tk, Tv, k=k).cpu().numpy(), want)


def test_knn_pruned_full_size_equals_brute_force(ops, monkeypatch):
    """BASELINE config 3 size (19 464 queries x 57 600 pixels): pruned == brute force, and fewer valid
    keys than k yields -1 like the brute-force path."""
    q, keys, valid = _knn_scene(5, 19464, 139)
    keys, valid = keys[:57600], valid[:57600]
    Tq, Tk, Tv = T(q), T(keys.reshape(3, 120, 160, 3)), T(valid.reshape(3, 120, 160))
    fast = ops.knn_pixels(Tq, Tk, Tv, k=3).cpu().numpy()
    few = valid.copy(); few[:] = False; few[[7, 5000]] = True
    fast_few = ops.knn_pixels(Tq, Tk, T(few.reshape(3, 120, 160)), k=3).cpu().numpy()
    monkeypatch.setenv("MVK_KNN_BRUTE", "1")
    assert np.array_equal(fast, ops.knn_pixels(Tq, Tk, Tv, k=3).cpu().numpy())
    assert np.array_equal(fast_few, ops.knn_pixels(Tq, Tk, T(few.reshape(3, 120, 160)), k=3).cpu().numpy())
    assert (fast_few[:, 2] == -1).all() and set(np.unique(fast_few[:, :2])) == {7, 5000}


def test_empty_and_degenerate_inputs(ops):
    kp = torch.zeros(15, 3, device="cuda")
    W = torch.zeros(15, 8, 4, device="cuda")
    q = torch.rand(10, 3, device="cuda")
    # no neighbour columns at all -> zeros
    y, _ = ops.kpconv(q, q, torch.zeros(10, 0, dtype=torch.int32, device="cuda"), torch.rand(10, 8, device="cuda"), kp, W, 0.1)
    assert y.shape == (10, 4) and float(y.abs().max()) == 0.0
    # no query points
    y, _ = ops.kpconv(q[:0], q, torch.zeros(0, 5, dtype=torch.int32, device="cuda"), torch.rand(10, 8, device="cuda"), kp, W, 0.1)
    assert y.shape == (0, 4)
    # a batch with an empty cloud on both sides
    nb = ops.radius_neighbors_batch(q, q, [0, 10], [0, 10], 0.5)
    assert nb.shape[0] == 10 and (nb[:, 0].cpu() == torch.arange(10, dtype=torch.int32)).all()
    sp, sl = ops.grid_subsample_batch(q, [0, 10, 0], dl=10.0)
    assert list(sl) == [0, 1, 0] and sp.shape == (1, 3)
    # gemm with an empty reduction
    assert float(ops.gemm(torch.zeros(3, 0, device="cuda"), torch.zeros(0, 2, device="cuda")).abs().max()) == 0.0


def test_capacity_errors_are_loud(ops):
    # more than 1024 in-range supports per query: LDS list capacity -> RuntimeError, never truncation
    s = torch.rand(3000, 3, device="cuda") * 0.01
    with pytest.raises(RuntimeError, match="in-range supports"):
        ops.radius_neighbors_batch(s[:4], s, [4], [3000], 1.0)
    # more than 64 distinct labels in one voxel
    p = torch.rand(500, 3, device="cuda") * 0.01
    lab = torch.arange(500, dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="distinct labels"):
        ops.grid_subsample_batch(p, [500], labels=lab, dl=1.0)
    with pytest.raises(RuntimeError, match="kernel size"):
        ops.kpconv(p, p, torch.zeros(500, 2, dtype=torch.int32, device="cuda"), torch.rand(500, 4, device="cuda"),
                   torch.zeros(17, 3, device="cuda"), torch.zeros(17, 4, 4, device="cuda"), 0.1)


def test_randomised_sweep_index_kernels_vs_oracle():
    """tools/fuzz_parity.py as a regression test: ragged batches (empty clouds included), lattice points
    (exact ties), features + labels, searches with and without a column limit, pruned vs brute-force 3-NN --
    12 seeded cases, zero mismatches against the CPU oracle."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "fuzz_parity.py"), "3", "12"], capture_output=True,
                       text=True, timeout=300, cwd=root)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "fuzz done, mismatches: 0" in p.stdout, p.stdout[-2000:]


# ------------------------------------------------------------------ degenerate inputs of the round-2 entry points

def test_round2_entry_points_on_empty_and_degenerate_inputs(ops):
    """Empty / all-padded inputs: a level with zero valid rows (capacity padding), a deformable layer without
    neighbours, a product with an empty reduction, an optimiser without gradients, an empty deferred list."""
    import mvkpconv
    optim = mvkpconv.sub("optim")
    # BatchNorm with n_valid = 0 (everything zero, no NaN) and with one valid row (variance 0, output = beta): the
    # single-launch kernel (300 rows) and the one fed by the GEMM's epilogue statistics (1 300 rows)
    B = torch.randn(64, 48, device="cuda")
    nv0 = torch.tensor([0], dtype=torch.int32, device="cuda")
    nv1 = torch.tensor([1], dtype=torch.int32, device="cuda")
    for rows in (300, 1300):
        A = torch.randn(rows, 64, device="cuda")
        bn = torch.nn.BatchNorm1d(48).cuda()
        y, st = ops.gemm(A, B, split_k=1, stats_n_valid=nv0)
        assert (st is not None) == (rows > ops.bn_single_launch_rows(48))
        if st is not None:
            y._mvk_bn_stats = st
        out = ops.bn_lrelu(y, nv0, bn, slope=0.1)
        assert torch.isfinite(out).all() and (out == 0).all() and torch.isfinite(bn.running_var).all()
        y, st = ops.gemm(A, B, split_k=1, stats_n_valid=nv1)
        if st is not None:
            y._mvk_bn_stats = st
        out = ops.bn_lrelu(y, nv1, bn, slope=1.0)
        assert torch.isfinite(out).all() and torch.allclose(out[0], bn.bias.detach(), atol=1e-6) and (out[1:] == 0).all()
    # product with an empty reduction / empty operands
    assert (ops.gemm(torch.zeros(5, 0, device="cuda"), torch.zeros(0, 7, device="cuda")) == 0).all()
    assert ops.gemm(torch.zeros(0, 4, device="cuda"), torch.zeros(4, 7, device="cuda")).shape == (0, 7)
    # deformable KPConv on a level without any neighbour column, forward and backward
    q = torch.rand(10, 3, device="cuda")
    x = torch.randn(10, 8, device="cuda", requires_grad=True)
    W = torch.randn(15, 8, 4, device="cuda", requires_grad=True)
    kp = torch.rand(15, 3, device="cuda") * 0.05
    off = torch.zeros(10, 15, 3, device="cuda", requires_grad=True)
    idx = torch.full((10, 3), 10, dtype=torch.int64, device="cuda")            # all shadow
    yk, md = ops.kpconv(q, q, idx, x, kp, W, 0.05, offsets=off)
    (yk.sum() + md.sum()).backward()
    assert (yk == 0).all() and torch.isfinite(md).all() and torch.isfinite(off.grad).all() and (x.grad == 0).all()
    # ... and with NO neighbour column at all (H == 0: the scatter returns before the offset-gradient kernel; the
    # offsets' gradient must then be zeros, not uninitialised memory -- ADVICE r2)
    for _ in range(3):
        junk = torch.full((10, 15, 3), float("nan"), device="cuda")            # poison what the allocator hands out next
        del junk
        off.grad = None
        yk, md = ops.kpconv(q, q, torch.zeros((10, 0), dtype=torch.int64, device="cuda"), x, kp, W, 0.05, offsets=off)
        yk.sum().backward()
        assert (yk == 0).all() and off.grad is not None and (off.grad == 0).all()
    # regulariser of an empty level
    l = ops.deform_regularizer(torch.zeros(0, 15, device="cuda"), torch.zeros(0, 15, 3, device="cuda"), 0.05, 1.2, 1.0)
    assert float(l) == 0.0
    # optimiser: no gradient anywhere -> nothing happens; deferred scope without products
    p = torch.nn.Parameter(torch.ones(9, device="cuda"))
    opt = optim.FusedClipSGD([p], lr=0.1, momentum=0.9, weight_decay=0.0, clip_value=1.0)
    opt.step()
    assert (p == 1).all()
    with ops.defer_weight_grads():
        pass


# ------------------------------------------------------------------ segmentation loss

@pytest.mark.parametrize("N,C,weighted,i64", [(19464, 20, False, True), (5000, 13, True, False), (300, 20, True, True),
                                              (1, 5, False, True), (70000, 20, False, False)])
def test_cross_entropy_lut_vs_torch(ops, N, C, weighted, i64):
    """csrc/loss.hip against the reference's formulation (architectures.py:345-372): labels outside valid_labels -> -1,
    CrossEntropyLoss(weight, ignore_index=-1) on the (1, C, N) logits; value and gradient; run twice (deterministic)."""
    torch.manual_seed(N + C)
    valid = np.sort(np.random.RandomState(C).choice(np.arange(0, C + 6), C, replace=False))       # raw label values
    top = int(valid.max())
    table = np.full(top + 3, -1, np.int64)
    for i, c in enumerate(valid):
        table[int(c) + 1] = i
    lut = torch.from_numpy(table).to("cuda", torch.int32)
    labels = torch.randint(-2, top + 4, (N,), device="cuda", dtype=torch.int64 if i64 else torch.int32)
    if N > 1:
        labels[0] = int(valid[0])                                  # at least one kept point
    else:
        labels[:] = int(valid[-1])
    x = (torch.randn(N, C, device="cuda") * 3).requires_grad_(True)
    w = (torch.rand(C, device="cuda") + 0.5) if weighted else None
    loss = ops.cross_entropy_lut(x, labels, lut, w)
    (g,) = torch.autograd.grad(loss * 1.7, x)
    loss2 = ops.cross_entropy_lut(x, labels, lut, w)
    assert float(loss.detach()) == float(loss2.detach())
    target = torch.from_numpy(table).cuda()[labels.long().clamp(-1, top + 1) + 1]
    xr = x.detach().clone().requires_grad_(True)
    ref = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1)(xr.t().unsqueeze(0), target.unsqueeze(0))
    (gr,) = torch.autograd.grad(ref * 1.7, xr)
    assert abs(float(loss.detach()) - float(ref.detach())) < 2e-6 * max(1.0, abs(float(ref.detach())))
    assert rel_err(g.cpu().numpy(), gr.cpu().numpy()) < 1e-5
    # every point ignored: NaN like torch's mean over nothing, gradient of the ignored rows zero
    none = ops.cross_entropy_lut(x, torch.full_like(labels, -1), lut, w)
    assert torch.isnan(none)


def test_fa_gather_reads_a_channels_last_map_in_place(ops):
    """mvk_fa_gather_fwd_ex: the (nv, C, h, w) map in channels-last memory gives the same X as its NCHW copy."""
    torch.manual_seed(3)
    nv, Cc, h, w, npts, k = 3, 64, 12, 16, 500, 3
    f = torch.randn(nv, Cc, h, w, device="cuda")
    xyz = torch.randn(nv, h, w, 3, device="cuda")
    pts = torch.randn(npts, 3, device="cuda")
    knn = torch.randint(0, nv * h * w, (npts, k), device="cuda")
    a = ops.fa_gather(f, xyz, knn, pts)
    fcl = f.contiguous(memory_format=torch.channels_last)
    assert not fcl.is_contiguous()
    b = ops.fa_gather(fcl, xyz, knn, pts)
    assert torch.equal(a, b)


@pytest.mark.parametrize("N,modulated", [(960, False), (257, True), (1, True), (5000, False)])
def test_deform_operands_kernel_vs_tensor_ops(ops, N, modulated):
    """mvk_deform_operands_fwd/bwd against the reference's tensor expression (blocks.py:243-266, :287): feat = raw +
    bias, offsets = feat[:, :3K] * extent, deformed_KP = offsets + kernel_points, modulations = 2 sigmoid(feat[:, 3K:]);
    gradients of raw and bias for gradients arriving on every output."""
    torch.manual_seed(N)
    K, ext = 15, 0.048
    D = (4 if modulated else 3) * K
    raw = torch.randn(N, D, device="cuda", requires_grad=True)
    bias = torch.randn(D, device="cuda", requires_grad=True)
    kp = torch.randn(K, 3, device="cuda")
    feat, off, dkp, mod = ops.deform_operands(raw, bias, kp, ext, modulated)
    go, gd, gf = torch.randn(N, K, 3, device="cuda"), torch.randn(N, K, 3, device="cuda"), torch.randn(N, D, device="cuda")
    loss = (off * go).sum() + (dkp * gd).sum() + (feat * gf).sum()
    gm = torch.randn(N, K, device="cuda")
    if modulated:
        loss = loss + (mod * gm).sum()
    g_raw, g_bias = torch.autograd.grad(loss, [raw, bias])
    r2, b2 = raw.detach().clone().requires_grad_(True), bias.detach().clone().requires_grad_(True)
    f2 = r2 + b2
    o2 = f2[:, :3 * K].reshape(-1, K, 3) * ext
    d2 = o2 + kp
    l2 = (o2 * go).sum() + (d2 * gd).sum() + (f2 * gf).sum()
    if modulated:
        m2 = 2 * torch.sigmoid(f2[:, 3 * K:])
        l2 = l2 + (m2 * gm).sum()
        assert rel_err(mod.detach().cpu().numpy(), m2.detach().cpu().numpy()) < 1e-6
    w_raw, w_bias = torch.autograd.grad(l2, [r2, b2])
    assert torch.equal(feat.detach(), f2.detach()) and torch.equal(off.detach(), o2.detach())
    assert torch.equal(dkp.detach(), d2.detach())
    assert rel_err(g_raw.cpu().numpy(), w_raw.cpu().numpy()) < 1e-6 and rel_err(g_bias.cpu().numpy(), w_bias.cpu().numpy()) < 1e-5
    # only the offsets receive a gradient (no regulariser, no modulation): the other inputs of the backward are absent
    (g_only,) = torch.autograd.grad((ops.deform_operands(raw, bias, kp, ext, modulated)[1] * go).sum(), [raw])
    assert rel_err(g_only[:, :3 * K].cpu().numpy(), (go.reshape(N, -1) * ext).cpu().numpy()) < 1e-6


def test_regulariser_of_all_layers_as_one_node_equals_the_per_layer_sum(ops):
    """ops.deform_regularizer_all (one accumulator, gradients scaled inside the backward launches) against the sum of
    the per-layer ops.deform_regularizer terms: value and every gradient, with an upstream factor other than 1."""
    torch.manual_seed(11)
    layers, leaves = [], []
    for N, ext in ((300, 0.05), (64, 0.1), (0, 0.2), (1000, 0.2)):
        m = torch.rand(N, 15, device="cuda").requires_grad_(True)
        d = (torch.randn(N, 15, 3, device="cuda") * ext).requires_grad_(True)
        nv = torch.tensor([max(N - 7, 0)], dtype=torch.int32, device="cuda") if N == 300 else None
        layers.append((m, d, ext, 1.2, 1.0, nv))
        leaves += [m, d]
    one = ops.deform_regularizer_all(layers)
    g_one = torch.autograd.grad(one * 0.37, leaves, allow_unused=True)
    per = sum(ops.deform_regularizer(m, d, ext, rep, pw, nv) for (m, d, ext, rep, pw, nv) in layers if m.shape[0] > 0)
    g_per = torch.autograd.grad(per * 0.37, leaves, allow_unused=True)
    assert abs(float(one.detach()) - float(per.detach())) < 1e-6 * max(1.0, abs(float(per.detach())))
    for a, b in zip(g_one, g_per):
        if b is None:
            assert a is None or a.numel() == 0
        else:
            assert rel_err(a.cpu().numpy(), b.cpu().numpy()) < 1e-6


@pytest.mark.parametrize("influence,agg", [("gaussian", "sum"), ("constant", "sum"), ("linear", "closest"), ("gaussian", "closest")])
@pytest.mark.parametrize("cin,idt", [(2, torch.int32), (4, torch.int64), (3, torch.int32)])
def test_kpconv_small_row_kernel_other_influences_vs_numpy_oracle(ops, cin, idt, influence, agg):
    """Rows of <= 4 channels with the non-default influence / aggregation modes, which kpconv_lane_channel<1, .., fwd>
    serves (one wave per point, two to four of its lanes hold a channel), and both index widths."""
    from oracle import npref
    rng = np.random.default_rng(cin * 7 + len(influence) + len(agg))
    Nq, Ns, K, H = 1001, 777, 15, 23
    q = (rng.random((Nq, 3)) * 0.3).astype(np.float32)
    s = (rng.random((Ns, 3)) * 0.3).astype(np.float32)
    idx = rng.integers(0, Ns + 1, (Nq, H))
    idx[7] = Ns
    x = rng.normal(size=(Ns, cin)).astype(np.float32)
    kp = (rng.normal(size=(K, 3)) * 0.05).astype(np.float32)
    W = (rng.normal(size=(K, cin, 5)) * 0.1).astype(np.float32)
    y, _ = ops.kpconv(T(q), T(s), torch.from_numpy(idx).to("cuda", idt), T(x), T(kp), T(W), 0.06, influence, agg)
    want = npref.kpconv_forward(q.astype(np.float64), s.astype(np.float64), idx.astype(np.int64), x.astype(np.float64),
                                kp.astype(np.float64), W.astype(np.float64), 0.06, influence, agg)
    assert rel_err(y.cpu().numpy(), want) < FP_TOL


def test_gradient_exchange_through_librccl_is_capturable_in_a_graph():
    """dp.RcclCommunicator + BucketedAllReduce(comm=...): pack, all-reduce on the exchange branch, unpack, captured in
    one hipGraph and replayed (one-rank communicator: the box has one GPU). Runs in a child process (process group)."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, os.path.join(root, "tools", "dp_graph_exchange_check.py")], capture_output=True,
                       text=True, timeout=300)
    assert p.returncode == 0 and "DP GRAPH EXCHANGE OK" in p.stdout, (p.stdout[-2000:], p.stderr[-3000:])
