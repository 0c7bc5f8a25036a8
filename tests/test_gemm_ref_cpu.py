"""CPU: the GEMM oracle of tests/gemm_ref.py is itself correct and its case lists reach what they claim.

  * every restatement equals torch float64 autograd of the literal expression;
  * every Family-I case satisfies its < 2^24 precondition, every Family-R case has no subnormal operand and a finite bound;
  * coverage is explicit: the path-choice restatement applied to the plain-product list proves every reachable loader
    pipeline x {0, 1, 2, 3, >= 4 full k-tiles} x {tail, no tail} per layout, every vector width by stride and by base
    offset, a ragged last split, and the tile edges of every tile class; what the host logic cannot reach is NAMED here;
  * the comparison rules reject what they should."""
import numpy as np
import pytest
import torch

import gemm_ref as ref

F64 = torch.float64


def t64(a, grad=False):
    return torch.tensor(np.asarray(a, np.float64), dtype=F64, requires_grad=grad)


def same(a, b):
    return np.array_equal(np.asarray(a, np.float64), np.asarray(b, np.float64))


# ------------------------------------------------------------------------------------------ restatements vs autograd

@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_product_restates_the_four_layouts_with_accumulate(layout):
    c = ref.Case(layout, 9, 11, 37, 0, 0, (2, 1, 1), "I", True)
    A, B, base = ref.operands(c)
    a, b = t64(A), t64(B)
    want = (a.t() if layout[0] == "T" else a) @ (b.t() if layout[1] == "T" else b)
    assert same(ref.product(A, B, layout), want.numpy())
    assert same(ref.product(A, B, layout, base), (want + t64(base)).numpy())
    Ar, Br, _ = ref.operands(c._replace(family="R", accumulate=False))
    a, b = t64(Ar), t64(Br)
    want = ((a.t() if layout[0] == "T" else a) @ (b.t() if layout[1] == "T" else b)).numpy()
    assert np.allclose(ref.product(Ar, Br, layout), want, rtol=1e-13, atol=0)


@pytest.mark.parametrize("slope", ref.BIAS_SLOPES)
def test_linear_bias_lrelu_restatement(slope):
    x, W, b, g = ref.bias_inputs(33, 20, 33)
    tx, tW, tb = t64(x, True), t64(W, True), t64(b, True)
    y = torch.nn.functional.leaky_relu(tx @ tW.t() + tb, slope)
    dx, dW, db = torch.autograd.grad(y, [tx, tW, tb], t64(g))
    r = ref.linear_bias_lrelu(x, W, b, slope, g)
    assert (r["pre"] == 0).any() and (r["pre"] < 0).any() and (r["pre"] > 0).any()
    assert same(r["y"], y.detach().numpy()) and same(r["dx"], dx.numpy()) and same(r["dW"], dW.numpy()) and same(r["db"], db.numpy())


def test_linear_pair_and_dual_restatements():
    x, W0, W1, g0, g1 = ref.pair_inputs(13, 7, 9, 21)
    tx, t0, t1 = t64(x, True), t64(W0, True), t64(W1, True)
    y0, y1 = tx @ t0.t(), tx @ t1.t()
    dx, d0, d1 = torch.autograd.grad([y0, y1], [tx, t0, t1], [t64(g0), t64(g1)])
    r = ref.linear_pair(x, W0, W1, g0, g1)
    for k, v in (("y0", y0.detach()), ("y1", y1.detach()), ("dx", dx), ("dW0", d0), ("dW1", d1)):
        assert same(r[k], v.numpy()), k
    A, B, A2, B2 = ref.dual_inputs(9, 11, 32, 5)
    assert same(ref.gemm_dual(A, B, A2, B2), (t64(A) @ t64(B) + t64(A2) @ t64(B2)).numpy())


@pytest.mark.parametrize("kind", ref.UPCAT_INDEX_KINDS)
def test_upsample_cat_linear_restatement(kind):
    x, idx, skip, W, g = ref.upcat_inputs(7, 40, 5, 3, 6, kind)
    assert idx.shape[1] == 3 and (idx[:, 1:] != idx[:, :1]).any()          # the other columns must not matter
    if kind == "random":
        assert (idx[:, 0] == 7).any() and (idx[:, 0] < 7).any()
    tx, ts, tW = t64(x, True), t64(skip, True), t64(W, True)
    xpad = torch.cat([tx, torch.zeros_like(tx[:1])], 0)
    y = torch.cat([xpad[torch.from_numpy(idx)[:, 0]], ts], 1) @ tW.t()
    dx, ds, dW = torch.autograd.grad(y, [tx, ts, tW], t64(g))
    r = ref.upsample_cat_linear(x, idx, skip, W, g)
    assert same(r["y"], y.detach().numpy()) and same(r["dx"], dx.numpy()) and same(r["dskip"], ds.numpy()) and same(r["dW"], dW.numpy())
    assert same(ref.upsample_cat_linear(x, idx[:, 0].astype(np.int32), skip, W, g)["dx"], dx.numpy())


def test_kp_ldb_and_passthrough_restatements():
    A2, W = ref.kp_inputs(9, 3, 5, 8)
    want = sum(t64(A2)[:, k, :] @ t64(W)[k].t() for k in range(3))
    assert same(ref.kp_transposed_contraction(A2, W), want.numpy())
    A, Bw = ref.ldb_inputs(9, 12, 17)
    assert same(ref.gemm_ldb(A, Bw, 2, 11), (t64(A) @ t64(Bw)[:, 2:13]).numpy())
    x, W, g, ga = ref.pass_inputs(9, 7, 12)
    for use_alias in (False, True):
        tx, tW = t64(x, True), t64(W, True)
        outs, grads = [tx @ tW.t()], [t64(g)]
        if use_alias:
            outs.append(tx.view_as(tx))
            grads.append(t64(ga))
        dx, dW = torch.autograd.grad(outs, [tx, tW], grads)
        r = ref.linear_passthrough(x, W, g, ga if use_alias else None)
        assert same(r["y"], outs[0].detach().numpy()) and same(r["dx"], dx.numpy()) and same(r["dW"], dW.numpy())


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 150])
def test_statistics_partials_restatement(n):
    A, B = ref.stats_inputs(150, 18, 33, "N")
    Cm = t64(ref.product(A, B))
    sums, m2, cnt = ref.stats_partials(Cm.numpy(), n, 64)
    assert sums.shape == (3, 18) and cnt.sum() == n
    for b in range(3):
        blk = Cm[64 * b:min(64 * b + 64, n)] if 64 * b < n else Cm[:0]
        assert cnt[b] == blk.shape[0]
        if blk.shape[0] == 0:
            assert not sums[b].any() and not m2[b].any()
        else:
            assert np.allclose(sums[b], blk.sum(0).numpy(), rtol=1e-13)
            assert np.allclose(m2[b], (blk.var(0, unbiased=False) * blk.shape[0]).numpy(), rtol=1e-9, atol=1e-9)
    assert np.isfinite(ref.m2_bound(m2, sums, cnt, 64)).all()


# ------------------------------------------------------------------------------------------ preconditions

def test_family_I_preconditions_and_family_R_operands():
    for c in ref.PLAIN_CASES:
        A, B, base = ref.operands(c)
        p = ref.path(*c[:6], force=c.force)
        ap = ref.abs_product(A, B, c.layout)
        if c.family == "I":
            for t in (A, B) + ((base,) if base is not None else ()):
                assert t.dtype == np.float32 and np.array_equal(t, np.rint(t)) and np.abs(t).max(initial=0) <= 4
            assert ref.precondition(ap, p.nsplit, base) < ref.EXACT_LIMIT, c
        else:
            assert base is None and not c.accumulate
            tiny = np.finfo(np.float32).tiny
            for t in (A, B):
                assert t.dtype == np.float32 and np.isfinite(t).all() and (np.abs(t) >= tiny).all(), c
            b = ref.r_bound(ap, c.K)
            assert np.isfinite(b).all() and (b > 0).all() and np.isfinite(ap.astype(np.float32)).all(), c


def test_family_I_preconditions_of_the_fused_forms():
    tops = []
    for M, N, K in ref.BIAS_SHAPES:
        x, W, b, g = ref.bias_inputs(M, N, K)
        r = ref.linear_bias_lrelu(x, W, b, 0.25, g)
        assert (r["pre"] == 0).any() and (r["pre"] < 0).any()                # both sides of the kink, and the kink itself
        tops.append(ref.top_magnitude(ref.linear_bias_lrelu(*(np.abs(t) for t in (x, W, b)), 1.0, np.abs(g))))
    for M, N0, N1, Kd, _ in ref.PAIR_CASES:
        tops.append(ref.top_magnitude(ref.linear_pair(*(np.abs(t) for t in ref.pair_inputs(M, N0, N1, Kd)))))
    for c in ref.DUAL_CASES:
        tops.append(ref.top_magnitude(ref.gemm_dual(*(np.abs(t) for t in ref.dual_inputs(*c)))))
    for c in ref.UPCAT_CASES:
        for kind in ref.UPCAT_INDEX_KINDS:
            x, idx, skip, W, g = ref.upcat_inputs(*c, kind)
            tops.append(ref.top_magnitude(ref.upsample_cat_linear(np.abs(x), idx, np.abs(skip), np.abs(W), np.abs(g))))
    for c in ref.KP_CASES:
        tops.append(ref.top_magnitude(ref.kp_transposed_contraction(*(np.abs(t) for t in ref.kp_inputs(*c)))))
    for M, Kd, col0, N, ldb, _ in ref.LDB_CASES:
        A, Bw = ref.ldb_inputs(M, Kd, ldb)
        assert ldb > col0 + N
        tops.append(ref.top_magnitude(ref.gemm_ldb(np.abs(A), np.abs(Bw), col0, N)))
    for M, N, K, _ in ref.STATS_CASES:
        A, B = ref.stats_inputs(M, N, K, "I")
        tops.append(M * ref.top_magnitude(ref.abs_product(A, B)))            # a column sum over every row
    for c in ref.DW_CASES + [ref.DW_SMALL]:
        A, B = ref.dw_inputs(*c)
        tops.append(ref.top_magnitude(ref.abs_product(A, B, "TN")))
    for c in ref.PASS_CASES:
        x, W, g, ga = (np.abs(t) for t in ref.pass_inputs(*c))
        tops.append(ref.top_magnitude(ref.linear_passthrough(x, W, g, ga)))
    assert max(tops) < ref.EXACT_LIMIT and min(tops) > 0


# ------------------------------------------------------------------------------------------ coverage

# What the host logic cannot reach through ops.gemm, by name:
UNREACHABLE = {
    "0 full k-tiles without a tail": "K = 0: no launch, the host zero-fills (the list still carries K = 0 per layout)",
    "pipeline (2,4) with a transposed A": "the row-contiguous fast loader is float4 only (Tile::fast_ok)",
    "pipeline (4,4) with a transposed A and M % 4 != 0": "the clamped float4 of the last rows needs whole float4 rows",
    "fewer than 4 full k-tiles per split in a split product": "plan_gemm drops an explicit split below 4 k-tiles per workgroup",
    "a requested split larger than the k-tile count": "same rule; LDB_CASES / DUAL_CASES reach clamp_split with one",
    "N = tile + 1 of a narrow class, N = 1 of the 32- / 64- / 128-column classes": "N itself selects the class",
}


def _paths():
    return [(c, ref.path(*c[:6], force=c.force)) for c in ref.PLAIN_CASES if c.K > 0]


def test_plain_list_covers_every_reachable_pipeline_tile_count_and_tail():
    seen = {(c.layout, p.pipeline, min(f, 4), tail) for c, p in _paths() for f, tail in p.parts}
    for layout in ref.LAYOUTS:
        assert any(c.layout == layout and c.K == 0 for c in ref.PLAIN_CASES)
        for pipe in ("44", "24", "general"):
            reach = pipe in ref.reachable_pipelines(layout)
            for full in (0, 1, 2, 3, 4):
                for tail in (False, True):
                    if full == 0 and not tail:
                        continue
                    assert ((layout, pipe, full, tail) in seen) == reach, (layout, pipe, full, tail)
    # the two unreachable pipeline classes really are: no shape of the restatement produces them
    for ta_layout in ("TN", "TT"):
        for M in range(1, 41):
            for oa in range(4):
                p = ref.path(ta_layout, M, 68, 64, oa, 0)
                assert p.pipeline != "24" and (p.pipeline != "44" or M % 4 == 0)
    assert any(c.layout == "NT" and p.pipeline == "24" for c, p in _paths())      # by the base offset alone
    # every split case keeps >= 4 k-tiles per workgroup, and asking for more splits than that runs unsplit
    assert all(min(f for f, _ in p.parts[:-1]) >= 4 for _, p in _paths() if p.nsplit > 1)
    assert ref.path("NN", 33, 68, 203, force=(2, 1, 3)).nsplit == 1 and ref.path("NN", 33, 68, 40, force=(2, 1, 3)).nsplit == 1
    assert ref.path("NN", 33, 68, 40, force=(2, 1, 3), explicit_request=False).nsplit == 2


def test_plain_list_covers_every_vector_width_by_stride_and_by_offset():
    have = set()
    for c, p in _paths():
        ta, tb = c.layout[0] == "T", c.layout[1] == "T"
        for name, vec, off, ld in (("A", p.vecA, c.offA, c.M if ta else c.K), ("B", p.vecB, c.offB, c.K if tb else c.N)):
            if vec == 4:
                have.add((name, 4, "aligned"))
            elif vec == 2:
                have.add((name, 2, "stride" if off % 4 == 0 else "offset" if ld % 4 == 0 else "both"))
            else:
                have.add((name, 1, "stride" if off % 4 == 0 else "offset" if ld % 4 == 0 else "both"))
    for name in "AB":
        assert {(name, 4, "aligned"), (name, 2, "stride"), (name, 2, "offset"), (name, 1, "stride"), (name, 1, "offset")} <= have
    assert {c.offA for c in ref.PLAIN_CASES} >= {0, 1, 2} and {c.offB for c in ref.PLAIN_CASES} >= {0, 1, 2}


def test_plain_list_covers_splits_and_tile_edges_of_every_class():
    paths = _paths()
    # a split whose last part is ragged (fewer k-tiles than the others, and one ending on a k-tail), ordered and atomic
    assert any(p.nsplit == 3 and p.parts[-1][0] < p.parts[0][0] for _, p in paths)
    assert any(p.nsplit > 1 and p.parts[-1][1] for _, p in paths)
    assert {p.nsplit for _, p in paths} >= {1, 2, 3}
    assert any(c.accumulate and p.nsplit > 1 for c, p in paths) and any(c.accumulate and p.nsplit == 1 for c, p in paths)
    classes = {(False, pm, qn) for pm, qn in ref.WIDE_FORCES} | {(True, pm, qn) for pm in (1, 2) for qn in (1, 2)}
    assert len(classes) == 11
    for c in ref.PLAIN_CASES:
        assert ref.launchable(c.N, c.force), c
    for layout in ref.LAYOUTS:                    # every forced plan x splits 1 / 2 / 3 in every layout
        for cls in classes:
            got = {p.nsplit for c, p in paths if c.layout == layout and (p.narrow, p.pm, p.qn) == cls}
            assert got >= {1, 2, 3}, (layout, cls)
    for narrow, pm, qn in classes:
        mine = [(c, p) for c, p in paths if (p.narrow, p.pm, p.qn) == (narrow, pm, qn)]
        tm, tn = mine[0][1].tm, mine[0][1].tn
        assert {c.M for c, _ in mine} >= {1, tm - 1, tm, tm + 1}, (narrow, pm, qn)
        want_n = {tn - 1, tn} | ({1} if tn == 16 else set()) | (set() if narrow else {tn + 1})
        assert {c.N for c, _ in mine} >= want_n, (narrow, pm, qn)
    assert len(UNREACHABLE) == 6


def test_fused_lists_hold_what_the_gpu_tests_promise():
    assert set(ref.BIAS_SHAPES) == {(M, N, K) for M in (1, 5, 33, 70) for N in (7, 20, 33, 64) for K in (16, 33, 64)}
    assert {(33, 64, 32, 1), (70, 68, 64, 33), (70, 128, 96, 100)} <= set(ref.DUAL_CASES)
    assert all(c[2] % ref.BK == 0 and c[1] > 32 for c in ref.DUAL_CASES)
    assert (ref.DUAL_NONE[0][2] == 48) and (ref.DUAL_NONE[1][1] == 20)
    assert {(7, 70, 4, 4, 64), (30, 100, 30, 7, 16), (5, 33, 64, 33, 48), (40, 200, 36, 28, 128)} <= set(ref.UPCAT_CASES)
    assert {(1, 1, 1, 32), (33, 3, 5, 32), (70, 15, 7, 64), (70, 2, 66, 128)} <= set(ref.KP_CASES) and any(c[3] == 45 for c in ref.KP_CASES)
    assert {(c[2], c[3]) for c in ref.LDB_CASES} >= {(c0, N) for c0 in (0, 1, 2, 4) for N in (4, 20, 64, 66)}
    assert any(s > ref.cdiv(Kd, ref.BK) for _, Kd, _, _, _, s in ref.LDB_CASES)          # more splits asked than k-tiles
    assert {c[2] for c in ref.DW_CASES} >= {17, 32, 33, 64, 130} and {c[0] for c in ref.DW_CASES} >= {1, 31, 33, 200, 1100}
    assert {c[1] for c in ref.DW_CASES} >= {1, 15, 64, 70} and ref.DW_SMALL[2] <= 16
    assert any(N0 == 32 and Kd <= 512 for _, N0, _, Kd, _ in ref.PAIR_CASES) and ref.PAIR_NONE[3] > 512 and ref.PAIR_NONE[1] <= 32
    assert any((N0, N1) == (48, 68) for _, N0, N1, _, _ in ref.PAIR_CASES)
    assert any(N0 > 32 and N1 > 32 for _, N0, N1, _, _ in ref.PAIR_CASES)


# ------------------------------------------------------------------------------------------ the rules reject

def test_exact_compare_rejects_small_faults():
    c = ref.Case("NN", 33, 68, 75, 0, 0, (2, 1, 1), "I", False)
    A, B, _ = ref.operands(c)
    want = ref.product(A, B)
    good = want.astype(np.float32)
    assert ref.exact(good, want)
    off = good.copy()
    off[17, 41] += 1
    assert not ref.exact(off, want)
    swapped = good.copy()
    swapped[[3, 4]] = swapped[[4, 3]]
    assert not np.array_equal(good[3], good[4]) and not ref.exact(swapped, want)
    k = int(np.argmax((A != 0).any(0) & (B != 0).any(1)))
    dropped = ref.product(np.delete(A, k, 1), np.delete(B, k, 0)).astype(np.float32)
    assert not ref.exact(dropped, want)
    nan = good.copy()
    nan[0, 0] = np.nan
    assert not ref.exact(nan, want) and not ref.exact(good[:, :-1], want)


def test_rounding_rule_rejects_a_small_element_and_accepts_float32():
    c = ref.Case("NN", 36, 68, 428, 0, 0, (2, 1, 1), "R", False)
    A, B, _ = ref.operands(c)
    want, ap = ref.product(A, B), ref.abs_product(A, B)
    f32 = A @ B                                                  # the float32 NumPy product of the same operands
    assert f32.dtype == np.float32 and ref.r_ratio(f32, want, ap, c.K) <= 1.0
    assert np.abs(want).max() / np.abs(want).min() > 1e8          # small and large outputs in one matrix
    i, j = np.unravel_index(np.argmin(ap), ap.shape)             # a small-magnitude element, off by 3 x ITS bound
    bad = want.copy()
    bad[i, j] += 3 * ref.r_bound(ap, c.K)[i, j]
    assert abs(bad[i, j] - want[i, j]) < 1e-5 * np.abs(want).max()        # far below what a max-norm measure resolves
    assert 2.9 < ref.r_ratio(bad, want, ap, c.K) < 3.1
    nan = want.copy()
    nan[0, 0] = np.nan
    assert ref.r_ratio(nan, want, ap, c.K) == np.inf
