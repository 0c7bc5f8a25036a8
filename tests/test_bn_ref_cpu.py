"""CPU: the float64 oracle of the masked BatchNorm (tests/bn_ref.py) against torch float64 autograd, the conditions its
case table must keep (in-band share, padded rows, n = 1), and the comparator itself: a float32 stand-in of the kernels
(shifted sums about row 0, pairwise summation) passes it on every case, and each of six single mutations of that
stand-in fails it on the tensors the mutation touches. The GPU side is tests/test_bn_oracle_gpu.py."""
import functools

import numpy as np
import pytest
import torch

import bn_ref as ref
from util import REFEREE_FACTOR, REFEREE_FLOOR

TOL = 1e-12
IDS = [ref.case_id(c) for c in ref.CASES]
BIG = ref.Case(19464, 64, 19000, "two")                 # the network's level-0 row count: comparator checks only
F = np.float32


@functools.lru_cache(maxsize=None)
def _inputs(c):
    return ref.inputs(c)


@functools.lru_cache(maxsize=None)
def _ref32(c):
    return ref.ref32_of_case(c, _inputs(c), "cpu")


def _t64(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).requires_grad_(grad)


# ------------------------------------------------------------------------------------ float32 stand-in of the kernels

def pairwise(a):
    """Column sums of a [n, D] float32 in float32, pairwise over the rows (NumPy's blocked pairwise sum runs along the
    contiguous axis)."""
    return np.sum(np.ascontiguousarray(a.T), axis=1, dtype=F)


def sequential(a):
    """The same sums with ONE accumulator per column, row after row."""
    out = np.zeros(a.shape[1], F)
    for row in a:
        out += row
    return out


def standin(c, inp, mutation=None, colsum=pairwise, updates=2):
    """What csrc/bn.hip computes, in NumPy float32: statistics as shifted sums about row 0, the LeakyReLU side from the
    sign of z (z <= 0 takes the slope), sums by `colsum`. mutation: one deliberate error (see MUTATIONS)."""
    R, D, n = c.R, c.D, c.n
    x, go, gamma, beta = inp["x"][:n], inp["go"][:n], inp["gamma"].copy(), inp["beta"]
    k = x[0]
    ns = n - 1 if mutation == "stats_drop_last_row" else n
    v = x[:ns] - k
    m1, m2 = colsum(v) / F(ns), colsum(v * v) / F(ns)
    mean = k + m1
    var = np.maximum(m2 - m1 * m1, F(0))
    invstd = (F(1) / np.sqrt(var + F(ref.EPS))).astype(F)
    xh = (x - mean) * invstd
    if mutation == "gamma_of_neighbour":
        gamma[-1] = gamma[-2]
    z = xh * gamma + beta
    if inp["addend"] is not None:
        z = z + inp["addend"][:n]
    low = z < 0 if mutation == "kink_excludes_zero" else z <= 0
    y = np.where(low, z * F(c.slope), z)
    gp = np.where(low, go * F(c.slope), go)
    dbeta, dgamma = colsum(gp), colsum(gp * xh)
    inv_n = F(1) / F(R if mutation == "dx_over_R" else n)
    dx = gamma * invstd * (gp - dbeta * inv_n - xh * dgamma * inv_n)
    unbiased = var if (n == 1 or mutation == "biased_running_var") else var * (F(n) / F(n - 1))
    rm, rv = ref.RUNNING0(D)
    m = F(ref.MOMENTUM)
    for _ in range(updates):
        rm, rv = (F(1) - m) * rm + m * mean, (F(1) - m) * rv + m * unbiased
    if mutation == "dgamma_dbeta_swapped":
        dgamma, dbeta = dbeta, dgamma
    out = {"y": y, "dx": dx, "d_addend": gp if inp["addend"] is not None else None, "dgamma": dgamma, "dbeta": dbeta,
           "mean": mean, "var": var, "running_mean": rm, "running_var": rv}
    assert all(a is None or a.dtype == F for a in out.values())
    return out


def _judge(c, inp, impl, r32, label):
    failures = {}
    report = ref.compare(label, impl, r32, ref.oracle_of_case(c, inp), failures)
    return failures, report


# ------------------------------------------------------------------------------------ the oracle itself

@pytest.mark.parametrize("c", ref.CASES, ids=IDS)
def test_oracle_equals_torch_float64_autograd(c):
    """F.batch_norm in double (+ addend) + leaky_relu and its autograd, y_impl = torch's own y: y, dx, dgamma, dbeta,
    d_addend within 1e-12 of the oracle's scales; the running statistics after two calls equal nn.BatchNorm1d.double()'s.
    One row (which torch's batch_norm refuses): the tensor expression in double."""
    inp, n = _inputs(c), c.n
    x, g, b = _t64(inp["x"][:n], True), _t64(inp["gamma"], True), _t64(inp["beta"], True)
    ad = _t64(inp["addend"][:n], True) if c.join else None
    if n > 1:
        z = torch.nn.functional.batch_norm(x, None, None, g, b, True, 0.0, ref.EPS)
    else:
        z = (x - x.mean(0)) * torch.rsqrt(x.var(0, unbiased=False) + ref.EPS) * g + b
    y = torch.nn.functional.leaky_relu(z + ad if c.join else z, c.slope)
    grads = torch.autograd.grad(y, [x, g, b] + ([ad] if c.join else []), _t64(inp["go"][:n]))
    got = {"y": y, "dx": grads[0], "dgamma": grads[1], "dbeta": grads[2], "d_addend": grads[3] if c.join else None}
    y_full = np.zeros((c.R, c.D))
    y_full[:n] = y.detach().numpy()
    o = ref.oracle_of_case(c, inp)(y_full)
    for name, t in got.items():
        if t is not None:
            assert ref.channel_errors(name, t.detach().numpy(), o).max() <= TOL, name
    if n > 1:
        bn = torch.nn.BatchNorm1d(c.D, momentum=ref.MOMENTUM).double()
        for _ in range(2):
            bn(x.detach())
        assert ref.channel_errors("running_mean", bn.running_mean.numpy(), o).max() <= TOL
        assert ref.channel_errors("running_var", bn.running_var.numpy(), o).max() <= TOL
        assert ref.channel_errors("mean", x.detach().mean(0).numpy(), o).max() <= TOL
        assert ref.channel_errors("var", x.detach().var(0, unbiased=False).numpy(), o).max() <= TOL


@pytest.mark.parametrize("c", ref.CASES, ids=IDS)
def test_in_band_share_is_below_the_cap(c):
    """At most BAND_SHARE_MAX of a case's valid elements sit where the LeakyReLU side is taken from the judged
    implementation (here a CPU float32 run). A case that breaks this gets another seed, not a wider cap."""
    inp = _inputs(c)
    y32 = _ref32(c)["y"] if c.n > 1 else standin(c, inp)["y"]
    y_full = np.zeros((c.R, c.D), F)
    y_full[:c.n] = y32
    share = ref.oracle_of_case(c, inp)(y_full).band_share
    print("%s: in-band share %.3e" % (ref.case_id(c), share))
    assert share <= ref.BAND_SHARE_MAX


@pytest.mark.parametrize("c", [c for c in ref.CASES if c.n < c.R], ids=lambda c: ref.case_id(c))
def test_padded_rows_are_exactly_zero(c):
    """Rows >= n of the oracle's y, dx, d_addend (and xh) are zero whatever y_impl holds there."""
    inp = _inputs(c)
    o = ref.oracle_of_case(c, inp)(np.ones((c.R, c.D)))
    for t in (o.y, o.dx, o.d_addend, o.xh):
        assert t.shape == (c.R, c.D) and not t[c.n:].any()


@pytest.mark.parametrize("join", [False, True])
def test_one_valid_row(join):
    """n = 1: variance 0, y = beta (+ addend) through the LeakyReLU, dx = 0, and the running variance takes the biased
    value (the kernels' rule; there is no unbiased one)."""
    c = ref.Case(5, 64, 1, "small", 0.1, join)
    inp = _inputs(c)
    z = inp["beta"].astype(np.float64) + (inp["addend"][0] if join else 0.0)
    y_full = np.zeros((c.R, c.D))
    y_full[0] = np.where(z > 0, z, 0.1 * z)
    o = ref.oracle_of_case(c, inp, updates=1)(y_full)
    assert not o.var.any() and not o.dx.any() and not o.xh.any() and not o.dgamma.any()
    assert np.array_equal(o.mean, inp["x"][0].astype(np.float64))
    assert np.abs(o.y[0] - y_full[0]).max() <= 1e-15
    assert np.allclose(o.running_var, 1 - ref.MOMENTUM, rtol=0, atol=1e-15)
    assert np.array_equal(o.d_addend[0], o.dbeta)


# ------------------------------------------------------------------------------------ the comparator can tell

@pytest.mark.parametrize("c", ref.CASES + (BIG,), ids=IDS + [ref.case_id(BIG)])
def test_float32_standin_passes_the_comparator(c):
    """Shifted sums about row 0 with pairwise summation: every tensor of every case inside the referee bound (the
    kernels sum 64-row blocks through a fixed tree, which is closer to this than to one accumulator per column)."""
    inp = _inputs(c)
    failures, report = _judge(c, inp, standin(c, inp), _ref32(c), "cpu stand-in " + ref.case_id(c))
    worst = max(e / b for e, b in report.values())
    print("%s: worst err / bound %.3f" % (ref.case_id(c), worst))
    assert not failures, failures


MUTATION_CASES = (ref.Case(50, 66, 37, "small", 0.1, True), ref.Case(600, 36, 577, "mid", 0.1, True))
# mutation -> the tensors it must break (at least)
MUTATIONS = {"dx_over_R": ("dx",), "stats_drop_last_row": ("y", "mean"), "biased_running_var": ("running_var",),
             "gamma_of_neighbour": ("y", "dx"), "dgamma_dbeta_swapped": ("dgamma", "dbeta")}


# every mutation on a small and a register-resident case; 1 / R for 1 / n also where the two differ by 1.2 % only
MUTATION_RUNS = [(m, c) for m in sorted(MUTATIONS) for c in MUTATION_CASES] + [("dx_over_R", ref.Case(8300, 32, 8200, "two"))]


@pytest.mark.parametrize("mutation,c", MUTATION_RUNS, ids=["%s-%s" % (m, ref.case_id(c)) for m, c in MUTATION_RUNS])
def test_single_mutations_of_the_standin_fail_the_comparator(mutation, c):
    """1 / R for 1 / n in dx; the last valid row left out of the statistics; biased running variance; the last
    channel's gamma taken from its neighbour (that channel alone may fail); dgamma and dbeta swapped."""
    inp = _inputs(c)
    failures, _ = _judge(c, inp, standin(c, inp, mutation), _ref32(c), "mutation %s %s" % (mutation, ref.case_id(c)))
    for name in MUTATIONS[mutation]:
        assert name in failures, (mutation, name, sorted(failures))
    if mutation == "gamma_of_neighbour":
        for name, channels in failures.items():
            assert list(channels) == [c.D - 1], (name, channels)
    if mutation == "dx_over_R":
        assert sorted(failures) == ["dx"]
    if mutation == "biased_running_var":
        assert sorted(failures) == ["running_var"]


@pytest.mark.parametrize("c", MUTATION_CASES, ids=lambda c: ref.case_id(c))
def test_slope_at_exactly_zero_is_seen_in_the_addend_gradient(c):
    """One element planted with z == 0 exactly (xh = 0, beta = 0, addend = 0; in float32 and float64 alike): the kernels
    give it the slope (z <= 0). A stand-in that gives the slope to z < 0 only returns the same y (0) and another
    d_addend; the oracle follows y_impl > 0 there and the comparator reports d_addend."""
    inp = {k: (v.copy() if v is not None else None) for k, v in _inputs(c).items()}
    n, ch, r0 = c.n, 3, 5
    assert n % 2 == 1
    col = np.full(n, 2.0, F)
    col[1::2] = 4.0                                  # rows 1, 3, ...: (n - 1) / 2 of them; rows 0, 2, ...: (n + 1) / 2
    col[r0 - 1] = 3.0                                # an even row: (n - 1) / 2 twos, (n - 1) / 2 fours, one three
    inp["x"][:n, ch], inp["beta"][ch], inp["addend"][r0 - 1, ch], inp["go"][r0 - 1, ch] = col, 0.0, 0.0, 1.0
    r32 = ref.ref32_of_case(c, inp, "cpu")
    good, bad = standin(c, inp), standin(c, inp, "kink_excludes_zero")
    assert good["y"][r0 - 1, ch] == 0 and bad["y"][r0 - 1, ch] == 0 and r32["y"][r0 - 1, ch] == 0
    assert good["d_addend"][r0 - 1, ch] == F(c.slope) and bad["d_addend"][r0 - 1, ch] == 1
    failures, _ = _judge(c, inp, good, r32, "planted zero, z <= 0 " + ref.case_id(c))
    assert not failures, failures
    failures, _ = _judge(c, inp, bad, r32, "planted zero, z < 0 " + ref.case_id(c))
    assert "d_addend" in failures and list(failures["d_addend"]) == [ch], failures


def test_one_accumulator_per_column_is_outside_the_bound_on_long_columns():
    """A warning for whoever changes the kernels' summation: the same stand-in with ONE float32 accumulator per column
    (row after row) leaves the bound on the 19 000-row case -- the referee bound is real, and what keeps the kernels
    inside it is their blocked, fixed-tree summation."""
    inp = _inputs(BIG)
    failures, report = _judge(BIG, inp, standin(BIG, inp, colsum=sequential), _ref32(BIG), "sequential stand-in " + ref.case_id(BIG))
    worst = {k: e / b for k, (e, b) in report.items()}
    print("sequential stand-in, err / bound:", {k: round(v, 3) for k, v in worst.items()})
    assert failures and max(worst.values()) > 1.0
    assert REFEREE_FACTOR == 3.0 and REFEREE_FLOOR == 1e-5        # the rule this file was written against
