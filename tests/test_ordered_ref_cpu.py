"""CPU: the NumPy oracle of the ordered pooling backwards (tests/ordered_ref.py) against torch float64 autograd of the
blocks.py restatement, its float32 walk against its float64 walk (the rounding level the GPU bounds are read against),
and the edges the case set must keep."""
import numpy as np
import pytest
import torch

import ordered_ref as ref
from util import bits_equal, check_err, rel_err

TOL = 1e-12


def _t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


@pytest.mark.parametrize("name", ref.CASES)
def test_oracle_equals_torch_float64_autograd(name):
    """max_pool: torch.cat([x, zeros_like(x[:1])])[idx].max(1); closest_pool: x_padded[idx[:, 0]]; and the sum over all
    columns of the gather (the full transposed relation). Forward values everywhere; max-pool gradients on the tie-free
    cases only (which of two equal columns torch.max routes to is not the contract)."""
    cs, C = ref.case(name), 5
    x, (g, base) = cs.features(C), cs.gradients(C)
    idx = torch.from_numpy(cs.idx)
    x64 = _t64(x, True)
    xp = torch.cat([x64, torch.zeros_like(x64[:1])], 0)
    pooled = xp[idx].max(1)[0]
    out, arg = ref.max_pool_fwd(x.astype(np.float64), cs.idx)
    assert np.array_equal(out, pooled.detach().numpy())
    out32, arg32 = ref.max_pool_fwd(x, cs.idx)                       # comparisons only: the same winners in float32
    assert np.array_equal(arg32, arg) and bits_equal(out32, out.astype(np.float32))
    if name in ref.TIE_FREE:
        (want,) = torch.autograd.grad(pooled, x64, _t64(g), retain_graph=True)
        got = ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, dtype=np.float64)
        assert rel_err(got, want.numpy()) < TOL
        got = ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, base=base, dtype=np.float64)
        assert rel_err(got, want.numpy() + base.astype(np.float64)) < TOL
    (want,) = torch.autograd.grad(xp[idx[:, 0]], x64, _t64(g), retain_graph=True)
    first = ref.reverse_lists(cs.idx, cs.Ns, first_column=True)
    assert rel_err(ref.gather_sum_rows(g, first, dtype=np.float64), want.numpy()) < TOL
    assert rel_err(ref.gather_sum_rows(g, first, base=base, dtype=np.float64), want.numpy() + base.astype(np.float64)) < TOL
    (want,) = torch.autograd.grad(xp[idx].sum(1), x64, _t64(g))
    full = ref.reverse_lists(cs.idx, cs.Ns)
    assert rel_err(ref.gather_sum_rows(g, full, dtype=np.float64), want.numpy()) < TOL


def test_reverse_lists_are_the_ascending_transposed_relation():
    cs = ref.case("h9")
    full, first = ref.reverse_lists(cs.idx, cs.Ns), ref.reverse_lists(cs.idx, cs.Ns, first_column=True)
    for j in range(cs.Ns):
        assert full[j] == [int(n) for n in np.nonzero((cs.idx == j).any(1))[0]]
        assert first[j] == [int(n) for n in np.nonzero(cs.idx[:, 0] == j)[0]]


@pytest.mark.parametrize("name", ["h7", "ties"])
def test_scatter_form_adds_in_the_order_of_the_plain_loop(name):
    """np.add.at over the query rows in their natural order = one float32 accumulator per element walked in ascending n:
    the vectorised sums of the oracle against the loop written out, bit for bit, with and without a start value."""
    cs, C = ref.case(name), 3
    x, (g, base) = cs.features(C), cs.gradients(C)
    _, arg = ref.max_pool_fwd(x, cs.idx)
    full = ref.reverse_lists(cs.idx, cs.Ns)
    for start in (None, base):
        gs = ref.gather_sum_rows(g, full, base=start)
        mp = ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, base=start)
        assert gs.dtype == np.float32 and mp.dtype == np.float32
        for c in range(C):
            s = None if start is None else start[:, c]
            want = ref.ordered_sum_loop(np.repeat(g[:, c], cs.H), cs.idx.reshape(-1), cs.Ns, s)
            assert bits_equal(gs[:, c], want)
            winners = cs.idx[np.arange(cs.Nq), arg[:, c]]
            assert bits_equal(mp[:, c], ref.ordered_sum_loop(g[:, c], winners, cs.Ns, s))


def test_float32_walk_against_float64_walk():
    """What rounding alone costs on these inputs: the ordered float32 sums against the same sums in float64, the largest
    rel_err over every case, width and sum. The GPU kernels are bit-equal to the float32 walk, so this is the figure their
    1e-6 bound against float64 is read against; the inputs are well conditioned as long as it stays below that bound."""
    worst = 0.0
    for name in ref.CASES:
        cs = ref.case(name)
        full, first = ref.reverse_lists(cs.idx, cs.Ns), ref.reverse_lists(cs.idx, cs.Ns, first_column=True)
        for C in (1, 10, 64):
            x, (g, base) = cs.features(C), cs.gradients(C)
            _, arg = ref.max_pool_fwd(x, cs.idx)
            for b in (None, base):
                pairs = [(ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, base=b, dtype=dt),
                          ref.gather_sum_rows(g, full, base=b, dtype=dt),
                          ref.gather_sum_rows(g, first, base=b, dtype=dt)) for dt in (np.float32, np.float64)]
                for a32, a64 in zip(*pairs):
                    assert a32.dtype == np.float32 and a64.dtype == np.float64
                    worst = max(worst, rel_err(a32, a64))
    check_err("ordered oracle: float32 walk vs float64 walk, worst over the case set", worst, 1e-6)
    assert worst > 0.0                        # (the float32 walk does round: the two are not one computation)


def test_an_empty_neighbourhood_pools_to_zero():
    cs = ref.case("h7")
    x, (g, base) = cs.features(4), cs.gradients(4)
    out, arg = ref.max_pool_fwd(x, cs.idx[:, :0])
    assert out.shape == (cs.Nq, 4) and not out.any() and not arg.any()
    assert bits_equal(ref.max_pool_bwd(g, arg, cs.idx[:, :0], cs.Ns, base=base), base)
    assert not ref.max_pool_bwd(g, arg, cs.idx[:, :0], cs.Ns).any()


def test_the_case_set_keeps_its_edges():
    """Every edge the GPU tests rely on is present, so an edit to the generator cannot lose one quietly."""
    seen = {k: False for k in ("empty reverse row", "reverse row of the full width", "all-shadow row",
                               "negative values beside a shadow entry", "negative values and no shadow entry",
                               "tie between two supports", "tie with the shadow row: support first",
                               "tie with the shadow row: shadow first")}
    assert sorted({ref.case(n).H for n in ref.CASES}) == [1, 7, 8, 9, 20]
    for name in ref.CASES:
        cs = ref.case(name)
        Ns, idx = cs.Ns, cs.idx
        assert idx.dtype == np.int64 and idx.min() >= 0 and idx.max() == Ns
        assert (idx[:, 0] == Ns).any() and (idx[:, 0] < Ns).any()          # shadow entries in column 0 too
        x, (g, _) = cs.features(10), cs.gradients(10)
        out, arg = ref.max_pool_fwd(x, idx)
        dx = ref.max_pool_bwd(g, arg, idx, Ns)
        xp = np.concatenate([x, np.zeros_like(x[:1])])
        for kind in (False, True):
            rows = ref.reverse_lists(idx, Ns, first_column=kind)
            lengths = np.asarray([len(r) for r in rows])
            width = lengths.max()                       # the width of an exact reverse list: its longest row fills it
            assert width >= 2 and (lengths < width).any()
            seen["empty reverse row"] |= bool(lengths[cs.unused] == 0)
            seen["reverse row of the full width"] |= bool((lengths == width).any())
        n = cs.rows["all_shadow"]
        assert (idx[n] == Ns).all() and not out[n].any() and not arg[n].any()
        seen["all-shadow row"] = True
        n = cs.rows["negative_and_shadow"]
        if n is not None:
            real = idx[n][idx[n] < Ns]
            assert 0 < real.size < cs.H and (x[real] < 0).all() and not out[n].any()
            assert (idx[n, arg[n]] == Ns).all()                          # the zero wins: the gradient goes nowhere
            seen["negative values beside a shadow entry"] = True
        n = cs.rows["negative_only"]
        assert (idx[n] < Ns).all() and (x[idx[n]] < 0).all() and (out[n] < 0).all()
        assert bits_equal(out[n], x[idx[n]].max(0))
        seen["negative values and no shadow entry"] = True
        gathered = xp[idx]                                                 # [Nq, H, C]
        ties = (gathered == out[:, None, :]).sum(1) > 1
        ties &= ~(idx == Ns).all(1)[:, None]
        if name in ref.TIE_FREE:
            # two shadow entries of one row tie trivially at zero and route nowhere either way; no other tie
            real_ties = ((gathered == out[:, None, :]) & (idx < Ns)[:, :, None]).sum(1)
            assert not ((real_ties > 1) | ((real_ties == 1) & (out == 0))).any()
            continue
        a, b = cs.tie_pair
        first_a = first_b = 0
        for n in range(20, 26):
            ca, cb = int(np.nonzero(idx[n] == a)[0][0]), int(np.nonzero(idx[n] == b)[0][0])
            assert ties[n].all() and (out[n] == x[a]).all() and (arg[n] == min(ca, cb)).all()
            first_a, first_b = first_a + (ca < cb), first_b + (cb < ca)
        assert first_a == 3 and first_b == 3                                 # (columns on both sides of the 8-wide trip)
        seen["tie between two supports"] = True
        z = cs.zero_support
        assert list(np.nonzero((idx == z).any(1))[0]) == [30, 31]
        assert not out[30].any() and (idx[30, arg[30]] == z).all() and bits_equal(dx[z], g[30])
        seen["tie with the shadow row: support first"] = True
        assert not out[31].any() and (idx[31, arg[31]] == Ns).all()
        seen["tie with the shadow row: shadow first"] = True
    assert all(seen.values()), seen
