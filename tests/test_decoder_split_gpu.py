"""GPU: the decoder's unary layer in its split form (ops._UpsampleCatLinearFn with ops.DECODER_SPLIT, csrc/gemm.hip:
the row-gathered addend of the NT product, the pair launch of two row counts, the output leading dimension of the
grouped weight-gradient launch) against the float64 restatement of tests/decoder_split_ref.py.
Bounds: those of test_gpu_parity.py::test_upsample_cat_linear_equals_the_three_steps -- 2e-6 on y, 5e-6 on the three
gradients (largest error over the largest reference magnitude)."""
import contextlib

import numpy as np
import pytest
import torch

import bn_ref
import decoder_split_ref as dref
from test_bn_oracle_gpu import check_run, dev, host, run_hip
from util import rel_err

pytestmark = pytest.mark.gpu

BOUND = {"y": 2e-6, "dx": 5e-6, "dskip": 5e-6, "dW": 5e-6}
NAMES = ("y", "dx", "dskip", "dW")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import mvkpconv
    o = mvkpconv.sub("ops")
    assert o.DECODER_SPLIT, "the split form is the default"
    return o


@contextlib.contextmanager
def deterministic(ops, flag):
    was = ops.is_deterministic()
    ops.set_deterministic(flag)
    try:
        yield
    finally:
        ops.set_deterministic(was)


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run(ops, data, Ns, idt=torch.int32, need_x=True, ordered=False, defer=False, stats_n=None):
    """One forward + backward of ops.upsample_cat_linear on fresh device tensors -> (y, dx, dskip, dW) device tensors
    (dx None when x takes no gradient) and the layer's output (for its statistics record)."""
    xh, idx, sh, Wh, gh = data
    x, skip, W, g = T(xh), T(sh), T(Wh), T(gh)
    inds = T(idx).to(idt)
    if ordered:
        ops.remember_reverse(inds, ops.reverse_neighbors(inds, Ns, first_column=True), first_column=True)
    x.requires_grad_(need_x), skip.requires_grad_(True), W.requires_grad_(True)
    nv = torch.tensor([stats_n], dtype=torch.int32, device="cuda") if stats_n is not None else None
    ops.step_begin()
    y = ops.upsample_cat_linear(x, inds, skip, W, stats_n_valid=nv)
    if defer:
        with ops.defer_weight_grads():
            (y * g).sum().backward()
    else:
        (y * g).sum().backward()
    return (y.detach(), x.grad, skip.grad, W.grad), y


def judge(label, got, want):
    errs = {}
    for name, t in zip(NAMES, got):
        if t is None:
            continue
        errs[name] = rel_err(t.cpu().numpy(), want[name])
    print(label, " ".join("%s %.2e" % kv for kv in errs.items()))
    for name, e in errs.items():
        assert e < BOUND[name], (label, name, e)


@pytest.mark.parametrize("case", dref.CASES, ids=str)
def test_split_form_vs_float64_every_index_form(ops, case):
    """int32 / int64 indices, 1-D / [Nq, 4] index matrices, a third of the rows on the shadow row; the weight gradient
    once in line and once through the grouped launch (two table entries into one tensor)."""
    Ns = case[0]
    for shadow in (False, True):
        for two_d in (False, True):
            data = dref.inputs(case, shadow, two_d)
            want = dref.split_form(*data)
            for idt in (torch.int32, torch.int64):
                for defer in (False, True):
                    got, _ = run(ops, data, Ns, idt, defer=defer)
                    judge("%s shadow=%d 2d=%d %s defer=%d" % (case, shadow, two_d, idt, defer), got, want)


def test_deep_reduction_case_splits_both_forward_products(ops):
    """(5, 40, 2048, 1024, 64): the coarse product and the product that carries the addend both split their reduction, so
    the addend must go in exactly once (test_split_form_vs_float64_every_index_form judges the values). The feature
    gradients reduce over the 64 output channels -- two k-tiles, which the plan never splits (it keeps four per
    workgroup)."""
    Ns, Nq, C1, C2, N = dref.CASES[1]
    assert ops.gemm_plan(Ns, N, C1)[0] > 1
    assert ops.gemm_plan(Nq, N, C2)[0] > 1
    assert ops.gemm_plan(Ns, C1, N)[0] == 1 and ops.gemm_plan(Nq, C2, N)[0] == 1


@pytest.mark.parametrize("case", dref.CASES, ids=str)
def test_split_form_when_the_coarse_features_take_no_gradient(ops, case):
    data = dref.inputs(case, shadow=True, two_d=True, seed=1)
    want = dref.split_form(*data)
    for ordered in (False, True):
        with deterministic(ops, ordered):
            got, _ = run(ops, data, case[0], need_x=False, ordered=ordered, defer=True)
        assert got[1] is None
        judge("%s no dx ordered=%d" % (case, ordered), got, want)


@pytest.mark.parametrize("case", dref.CASES, ids=str)
def test_ordered_mode_is_bit_reproducible_and_inside_the_bounds(ops, case):
    data = dref.inputs(case, shadow=True, two_d=True, seed=2)
    want = dref.split_form(*data)
    with deterministic(ops, True):
        a, _ = run(ops, data, case[0], ordered=True, defer=True)
        b, _ = run(ops, data, case[0], ordered=True, defer=True)
    judge("%s ordered" % (case,), a, want)
    for name, s, t in zip(NAMES, a, b):
        assert torch.equal(s, t), name


@pytest.mark.parametrize("case", dref.CASES, ids=str)
def test_split_and_concatenated_forms_agree_inside_the_bounds(ops, case, monkeypatch):
    data = dref.inputs(case, shadow=True, seed=3)
    want = dref.split_form(*data)
    got1, _ = run(ops, data, case[0])
    monkeypatch.setattr(ops, "DECODER_SPLIT", False)
    got0, _ = run(ops, data, case[0])
    judge("%s split" % (case,), got1, want)
    judge("%s concatenated" % (case,), got0, want)


@pytest.mark.parametrize("case", dref.CASES + dref.STATS_CASES, ids=str)
def test_statistics_of_the_valid_rows_behind_the_split_form(ops, case):
    """stats_n_valid < Nq: the BatchNorm that follows (ops.bn_lrelu) takes the layer's epilogue partials where the product
    carries them (the two STATS_CASES) and its own statistics pass elsewhere; either way mean and variance of the valid
    rows, forward and backward, under the referee rule of tests/test_bn_oracle_gpu.py against the float64 oracle of the
    float32 output."""
    Ns, Nq, C1, C2, N = case
    n = Nq - 37
    data = list(dref.inputs(case, shadow=True, seed=4))
    # skip features about 1 instead of 0: the column means of y are then a fair fraction of its spread. The referee scales
    # the error of running_mean by |mean| itself (tests/bn_ref.py), so a channel whose mean happens to lie within a percent
    # of a standard deviation of zero is judged on rounding noise -- of the BatchNorm kernel, not of this layer.
    data[2] = data[2] + np.float32(1.0)
    got, y = run(ops, data, Ns, stats_n=n)
    judge("%s stats" % (case,), got, dref.split_form(*data))
    st = ops.bn_stats_of(y)
    if case in dref.STATS_CASES:
        assert st is not None and st.partials.shape == ((Nq + st.rows - 1) // st.rows, 2, N)
        # the partial sums are float32 sums of st.rows accumulator values each (the addend already inside): against the
        # float64 column sums of the float32 output over the valid rows, (rows + 8) 2^-24 of the summed magnitudes
        sums = st.partials[:, 0, :].double().sum(0).cpu().numpy()
        yv = host(y).astype(np.float64)[:n]
        assert (np.abs(sums - yv.sum(0)) <= (st.rows + 8) * 2.0 ** -24 * np.abs(yv).sum(0)).all()
        # and the float64 restatement's own sums, as far as y itself is held to it
        want = dref.split_form(*data, n_valid=n)
        assert np.abs(sums - want["stat_sum"]).max() <= n * BOUND["y"] * np.abs(want["y"]).max() + \
            ((st.rows + 8) * 2.0 ** -24 * np.abs(yv).sum(0)).max()
    rng = np.random.default_rng(Nq + N)
    f = np.float32
    gamma, beta = rng.uniform(0.5, 1.5, N).astype(f), rng.uniform(-0.5, 0.5, N).astype(f)
    go = rng.standard_normal((Nq, N)).astype(f)
    x = y.detach()
    if st is not None:
        x._mvk_bn_stats = st
    x.requires_grad_(True)
    out, first, counter = run_hip(ops, x, n, dev(gamma), dev(beta), 0.1, None, dev(go))
    xh = host(y)
    run0 = bn_ref.RUNNING0(N)
    oracle_of = lambda yy: bn_ref.oracle(xh, n, gamma, beta, bn_ref.EPS, 0.1, None, go, yy, run0, bn_ref.MOMENTUM, 2)
    r32 = bn_ref.ref32(xh, n, gamma, beta, bn_ref.EPS, 0.1, None, go, run0, bn_ref.MOMENTUM, 2, "cuda")
    check_run("bn behind the split decoder layer %s" % (case,), out, first, counter, n, r32, oracle_of)


@pytest.mark.parametrize("Kd,M,n0,n1", [(70, 20, 24, 40), (2000, 64, 96, 33)])
def test_grouped_launch_writes_only_its_column_windows(ops, Kd, M, n0, n1):
    """The output leading dimension of the grouped weight-gradient launch on its own: two TN products A^T B into two
    column windows of one sentinel-filled tensor through defer_weight_grads, one short reduction (plain stores) and one
    the grouped plan splits (atomics onto zero-filled windows). The windows hold the dense products, every column
    outside them still holds the sentinel."""
    rng = np.random.default_rng(Kd + M)
    A0, B0 = rng.normal(size=(Kd, M)).astype(np.float32), rng.normal(size=(Kd, n0)).astype(np.float32)
    A1, B1 = rng.normal(size=(Kd + 5, M)).astype(np.float32), rng.normal(size=(Kd + 5, n1)).astype(np.float32)
    lo, gap, hi = 3, 5, 2
    ld = lo + n0 + gap + n1 + hi
    w0, w1 = lo, lo + n0 + gap
    for ordered in (False, True):
        with deterministic(ops, ordered):
            split = ops.lib().mvk_gemm_f32_tn_grouped_split(M, n0, Kd)
            assert (split > 1) == (Kd > 512)
            out = torch.full((M, ld), -7.0, device="cuda")
            out[:, w0:w0 + n0] = 0
            out[:, w1:w1 + n1] = 0
            ops.step_begin()
            with ops.defer_weight_grads():
                st = out.untyped_storage()
                for A, B, w in ((T(A0), T(B0), w0), (T(A1), T(B1), w1)):
                    ops._DEFER["items"].append((A, B, out.data_ptr() + 4 * w, True, st, ld))
            res = out.cpu().numpy()
        assert rel_err(res[:, w0:w0 + n0], A0.astype(np.float64).T @ B0.astype(np.float64)) < 5e-6
        assert rel_err(res[:, w1:w1 + n1], A1.astype(np.float64).T @ B1.astype(np.float64)) < 5e-6
        keep = np.ones(ld, bool)
        keep[w0:w0 + n0] = keep[w1:w1 + n1] = False
        assert (res[:, keep] == -7.0).all()
