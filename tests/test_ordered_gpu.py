"""GPU: the backward kernels that only ops.set_deterministic(True) runs, held to an ordered oracle.

The gather-form backwards of max_pool, closest_pool and the decoder's upsampling (csrc/revlist.hip) do nothing but
float32 additions in a fixed order, so they must give the BITS of tests/ordered_ref.py walked in np.float32, and stay
within the default mode's bound of the float64 walk. The ordered bias sum (csrc/bn.hip), the serial regulariser and the
one-workgroup deform-operand backward (csrc/deform.hip) multiply before they add: they are held to float64 with the bound
their default-mode tests use. A module fixture turns the mode on and makes a missing reverse list an error, so no test
here can pass on the atomic fall-back. The elementwise add_lrelu and bias_act_nhwc ride along (no mode dependence)."""
import contextlib
import functools
import itertools

import numpy as np
import pytest
import torch

import ordered_ref as ref
from test_gpu_parity import regulariser_float64
from util import bits_equal, check_err, rel_err

pytestmark = pytest.mark.gpu

POOL_BOUND = 1e-6          # test_pools_golden, test_upsample_cat_equals_closest_pool_then_cat (default mode, same operators)
CAT_LINEAR_BOUND = 5e-6    # test_upsample_cat_linear_equals_the_three_steps: its three gradients
CAT_LINEAR_FWD = 2e-6      # the same test's bound on the layer's output
DBIAS_BOUND = 1e-5         # test_bias_lrelu_vs_torch; also d_bias of test_deform_operands_kernel_vs_tensor_ops
REG_BOUND = 1e-5           # test_deform_regularizer_kernel_vs_reference_formula
D_RAW_BOUND = 1e-6         # test_deform_operands_kernel_vs_tensor_ops


@pytest.fixture(scope="module")
def ops():
    import mvkpconv
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return mvkpconv.sub("ops")


@pytest.fixture(scope="module", autouse=True)
def ordered_mode(ops):
    """Deterministic mode for the whole module; a scatter without a reverse list raises instead of taking the atomic
    path (which is also correct, and warns once per process: the ordered kernel would go untested in silence)."""
    def refuse(what):
        raise AssertionError("deterministic mode found no reverse list for %s: the atomic path would have run" % what)

    was = ops.is_deterministic()
    patch = pytest.MonkeyPatch()
    ops.set_deterministic(True)
    try:
        assert ops.is_deterministic() and ops.lib().mvk_gemm_split_ordered() == 1
        patch.setattr(ops, "_no_reverse_list", refuse)
        yield
    finally:
        patch.undo()
        ops.set_deterministic(was)


@contextlib.contextmanager
def atomic_mode(ops):
    ops.set_deterministic(False)
    try:
        assert not ops.is_deterministic() and ops.lib().mvk_gemm_split_ordered() == 0
        yield
    finally:
        ops.set_deterministic(True)
        assert ops.is_deterministic() and ops.lib().mvk_gemm_split_ordered() == 1


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def f64(a):
    return np.asarray(a, np.float64)


@functools.lru_cache(maxsize=None)
def the_case(name):
    return ref.case(name)


@functools.lru_cache(maxsize=None)
def the_lists(name, first_column):
    cs = the_case(name)
    return ref.reverse_lists(cs.idx, cs.Ns, first_column=first_column)


def reverse_on_device(ops, inds, Ns, lists, first_column, capacity=False):
    """ops.reverse_neighbors (sorted) checked against the oracle's lists; capacity: written into a matrix with more rows
    than Ns and more columns than the longest row, as a capacity-padded batch holds it."""
    width = max(max(len(r) for r in lists), 1)
    if capacity:
        rev = torch.full((Ns + 37, width + 5), -7, dtype=torch.int32, device="cuda")
        ops.reverse_neighbors(inds, Ns, out=rev, sort=True, first_column=first_column)
    else:
        rev = ops.reverse_neighbors(inds, Ns, sort=True, first_column=first_column)
        assert rev.shape == (Ns, width)
    got, shadow = host(rev), inds.shape[0]
    for j, r in enumerate(lists):
        assert list(got[j, :len(r)]) == r and (got[j, len(r):] == shadow).all(), j
    return rev


# ------------------------------------------------------------------------------------------------ a. gather_sum_rows

LAYOUTS = {"contiguous": None, "block at 0": (0, 0), "block at 4": (4, 0), "block at 1": (1, 0), "odd row stride": (0, 1)}


def column_block(g, layout):
    """g [Nq, C] on the device: dense, or as the columns [start, start + C) of a wider tensor whose row stride is a
    multiple of four (the float4 loads; from an offset pointer; from a pointer that is not 16-byte aligned) or is not."""
    if LAYOUTS[layout] is None:
        return dev(g)
    start, odd = LAYOUTS[layout]
    Nq, C = g.shape
    ld = (start + C + 3) // 4 * 4 + 4 + odd
    wide = np.random.default_rng(ld).standard_normal((Nq, ld)).astype(np.float32)
    wide[:, start:start + C] = g
    view = dev(wide)[:, start:start + C]
    assert view.stride() == (ld, 1) and view.data_ptr() % 16 == (4 * start) % 16 and (ld % 4 != 0) == bool(odd)
    return view


@pytest.mark.parametrize("C", [1, 3, 4, 7, 30, 64, 66])
@pytest.mark.parametrize("name,first_column", [("h7", False), ("h8", True), ("h20", False)])
def test_gather_sum_rows_adds_in_ascending_row_order(ops, name, first_column, C):
    """mvk_gather_sum_rows called directly: Ns = 70 and 300, up to 1 200 query rows, reverse rows from empty to the full
    width; every load path (float4, float4 from an offset block, scalar for a misaligned pointer, scalar for a row stride
    that is no multiple of four, ragged last four channels), with and without a start value, exact and capacity-padded
    reverse matrix -- all the same bits as the float32 walk, and within the pool bound of the float64 walk."""
    cs, lists = the_case(name), the_lists(name, first_column)
    g, base = cs.gradients(C)
    inds = dev(cs.idx)
    revs = {"exact": reverse_on_device(ops, inds, cs.Ns, lists, first_column),
            "capacity": reverse_on_device(ops, inds, cs.Ns, lists, first_column, capacity=True)[:cs.Ns]}
    assert revs["capacity"].shape[1] > revs["exact"].shape[1] and revs["capacity"].is_contiguous()
    worst = 0.0
    for b in (None, base):
        want = ref.gather_sum_rows(g, lists, base=b)
        worst = max(worst, rel_err(want, ref.gather_sum_rows(g, lists, base=b, dtype=np.float64)))
        for layout, form in itertools.product(LAYOUTS, revs):
            got = ops.gather_sum_rows(column_block(g, layout), revs[form], None if b is None else dev(b))
            assert bits_equal(host(got), want), (layout, form, b is not None)
    check_err("ordered gather_sum_rows %s%s C=%d vs float64" % (name, " col 0" if first_column else "", C), worst, POOL_BOUND)


# ------------------------------------------------------------------------------------------------ b. upsampling

UP_SHAPES = [(300, 1000, 30, 7, 16), (85, 332, 64, 32, 64), (70, 260, 4, 4, 8)]


def upsampling_problem(ops, Ns, Nq, C1, C2, Cout, idt):
    rng = np.random.default_rng(Ns + C1)
    idx = ref.index_matrix(Ns, Nq, 4, seed=Nq)
    assert (idx[:, 0] == Ns).any() and (idx[:, 0] < Ns).any()
    lists = ref.reverse_lists(idx, Ns, first_column=True)
    inds = dev(idx).to(idt)
    ops.remember_reverse(inds, reverse_on_device(ops, inds, Ns, lists, True), first_column=True)
    x = rng.standard_normal((Ns, C1)).astype(np.float32)
    skip = rng.standard_normal((Nq, C2)).astype(np.float32)
    W = (rng.standard_normal((Cout, C1 + C2)) * 0.05).astype(np.float32)
    up = np.concatenate([x, np.zeros_like(x[:1])])[idx[:, 0]]                 # blocks.py:88-91
    return rng, idx, lists, inds, x, skip, W, up


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("Ns,Nq,C1,C2,Cout", UP_SHAPES)
def test_closest_pool_and_upsample_cat_backwards_are_the_ordered_sums(ops, Ns, Nq, C1, C2, Cout, idt):
    """closest_pool alone, closest_pool behind torch.cat (its gradient arrives as a column block of the wider one and is
    read in place) and the fused upsample_cat: forward bits, dx = the float32 walk over the first-column relation bit for
    bit, d_skip = the gradient's other column block."""
    rng, idx, lists, inds, x, skip, W, up = upsampling_problem(ops, Ns, Nq, C1, C2, Cout, idt)
    g = rng.standard_normal((Nq, C1 + C2)).astype(np.float32)
    want = ref.gather_sum_rows(g[:, :C1], lists)
    check_err("ordered closest_pool dx Ns=%d C1=%d vs float64" % (Ns, C1),
              rel_err(want, ref.gather_sum_rows(g[:, :C1], lists, dtype=np.float64)), POOL_BOUND)
    xt, st, gt = dev(x).requires_grad_(True), dev(skip).requires_grad_(True), dev(g)
    alone = ops.closest_pool(xt, inds)
    assert bits_equal(host(alone), up)
    (dx,) = torch.autograd.grad(alone, xt, dev(g[:, :C1]))
    assert bits_equal(host(dx), want)
    behind_cat = torch.cat([ops.closest_pool(xt, inds), st], dim=1)
    fused = ops.upsample_cat(xt, inds, st)
    assert bits_equal(host(fused), np.concatenate([up, skip], 1)) and torch.equal(fused, behind_cat)
    for out in (behind_cat, fused):
        dx, ds = torch.autograd.grad(out, [xt, st], gt)
        assert bits_equal(host(dx), want) and bits_equal(host(ds), g[:, C1:])


@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("Ns,Nq,C1,C2,Cout", UP_SHAPES)
def test_upsample_cat_linear_ordered_backward_vs_float64(ops, Ns, Nq, C1, C2, Cout, idt):
    """The decoder's upsampling + concatenation + unary layer in deterministic mode: dx = (ordered row sums of g) .
    W[:, :C1], d_skip = g . W[:, C1:] (both through mvk_gemm_f32_ldb) and dW, against float64 with the row sums taken
    first; two backward runs give the same bits."""
    rng, idx, lists, inds, x, skip, W, up = upsampling_problem(ops, Ns, Nq, C1, C2, Cout, idt)
    g = rng.standard_normal((Nq, Cout)).astype(np.float32)
    cat64, W64, g64 = f64(np.concatenate([up, skip], 1)), f64(W), f64(g)
    xt, st, Wt = (dev(a).requires_grad_(True) for a in (x, skip, W))
    ops.step_begin()
    y = ops.upsample_cat_linear(xt, inds, st, Wt)
    label = "ordered upsample_cat_linear Ns=%d C1=%d %s " % (Ns, C1, str(idt)[6:])
    check_err(label + "y vs float64", rel_err(host(y), cat64 @ W64.T), CAT_LINEAR_FWD)
    runs = [torch.autograd.grad(y, [xt, st, Wt], dev(g), retain_graph=True) for _ in range(2)]
    for a, b in zip(*runs):
        assert torch.equal(a, b)
    dx, ds, dW = (host(t) for t in runs[0])
    check_err(label + "dx vs float64", rel_err(dx, ref.gather_sum_rows(g, lists, dtype=np.float64) @ W64[:, :C1]), CAT_LINEAR_BOUND)
    check_err(label + "d_skip vs float64", rel_err(ds, g64 @ W64[:, C1:]), CAT_LINEAR_BOUND)
    check_err(label + "dW vs float64", rel_err(dW, g64.T @ cat64), CAT_LINEAR_BOUND)


@pytest.mark.parametrize("M,Kd,C1,C2", [(1000, 16, 30, 7), (332, 64, 64, 32), (85, 8, 4, 4)])
def test_gemm_ldb_reads_a_column_block_in_place(ops, M, Kd, C1, C2):
    """ops.gemm_ldb(A, W, col0, N, ldb) = A @ W[:, col0:col0 + N] for both halves of the decoder's g . W (the second
    starts at a pointer that is not 16-byte aligned when C1 % 4 != 0), against float64."""
    rng = np.random.default_rng(M + Kd)
    A = rng.standard_normal((M, Kd)).astype(np.float32)
    W = (rng.standard_normal((Kd, C1 + C2)) * 0.05).astype(np.float32)
    ops.step_begin()
    for col0, N in ((0, C1), (C1, C2)):
        got = ops.gemm_ldb(dev(A), dev(W), col0, N, C1 + C2)
        assert got.shape == (M, N)
        check_err("ordered gemm_ldb M=%d Kd=%d col0=%d N=%d vs float64" % (M, Kd, col0, N),
                  rel_err(host(got), f64(A) @ f64(W)[:, col0:col0 + N]), CAT_LINEAR_BOUND)


# ------------------------------------------------------------------------------------------------ c. max_pool

@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
@pytest.mark.parametrize("C", [1, 10, 64])
@pytest.mark.parametrize("name", ref.CASES)
def test_max_pool_forward_and_both_backwards(ops, name, C, idt):
    """max_pool over pooling matrices of H = 1, 7, 8, 9, 20 columns with all-shadow rows, negative rows beside and without
    a shadow entry and exact ties (which must go to the first column). Forward: the oracle's bits. Deterministic
    backward (mvk_max_pool_bwd_gather): the float32 walk bit for bit -- alone, on top of a second consumer's gradient
    (passthrough: the kernel's `base`), with a capacity-padded reverse matrix, twice. Then the default mode's atomic
    scatter, with its in-place accumulation onto the alias gradient, against the float64 walk."""
    cs, lists = the_case(name), the_lists(name, False)
    x, (g, base) = cs.features(C), cs.gradients(C)
    out, arg = ref.max_pool_fwd(x, cs.idx)
    want = ref.max_pool_bwd(g, arg, cs.idx, cs.Ns)
    base15 = base * np.float32(1.5)                                     # what the second consumer sends back
    want_base = ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, base=base15)
    w64, w64_base = (ref.max_pool_bwd(g, arg, cs.idx, cs.Ns, base=b, dtype=np.float64) for b in (None, base15))
    label = "max_pool %s C=%d %s " % (name, C, str(idt)[6:])
    check_err(label + "ordered dx vs float64", max(rel_err(want, w64), rel_err(want_base, w64_base)), POOL_BOUND)
    xt, gt, bt = dev(x).requires_grad_(True), dev(g), dev(base)

    def run(inds):
        pooled = ops.max_pool(xt, inds)
        assert bits_equal(host(pooled), out)
        (dx,) = torch.autograd.grad(pooled, xt, gt)
        pooled, alias = ops.max_pool(xt, inds, passthrough=True)
        assert bits_equal(host(pooled), out) and alias.data_ptr() == xt.data_ptr()
        (dx_base,) = torch.autograd.grad([pooled, alias * 1.5], xt, [gt, bt])
        pooled, alias = ops.max_pool(xt, inds, passthrough=True)         # only the alias is used: its gradient passes
        (only,) = torch.autograd.grad(alias * 1.5, xt, bt)
        assert bits_equal(host(only), base15)
        return host(dx), host(dx_base)

    inds = dev(cs.idx).to(idt)
    ops.remember_reverse(inds, reverse_on_device(ops, inds, cs.Ns, lists, False))
    first = run(inds)
    assert bits_equal(first[0], want) and bits_equal(first[1], want_base)
    again = run(inds)
    assert bits_equal(again[0], first[0]) and bits_equal(again[1], first[1])
    padded = dev(cs.idx).to(idt)                                          # the same matrix, a capacity-padded reverse list
    ops.remember_reverse(padded, reverse_on_device(ops, padded, cs.Ns, lists, False, capacity=True))
    wide = run(padded)
    assert bits_equal(wide[0], want) and bits_equal(wide[1], want_base)
    with atomic_mode(ops):
        ops.step_begin()
        dx, dx_base = run(dev(cs.idx).to(idt))                            # (no reverse list registered, none needed)
    check_err(label + "atomic dx vs float64", rel_err(dx, w64), POOL_BOUND)
    check_err(label + "atomic dx onto the alias gradient vs float64", rel_err(dx_base, w64_base), POOL_BOUND)


# ------------------------------------------------------------------------------------------------ d. ordered bias sum

BIAS_SHAPES = [(1, 7, 0.1), (300, 1, 0.1), (1100, 256, 0.1), (4200, 20, 0.1), (5000, 128, 0.1), (5000, 128, 1.0)]


@pytest.mark.parametrize("R,C,slope", BIAS_SHAPES)
def test_bias_lrelu_ordered_bias_gradient(ops, R, C, slope):
    """mvk_bias_lrelu_bwd with the arena set: the workgroups park their column sums and the last one adds them in
    workgroup order ((300, 1): 256 row lanes over 5 workgroups; (1100, 256): one row lane, 18 workgroups, i.e. a second,
    clamped round of sixteen loads; (4200, 20): 8 row lanes, 66 workgroups). y and dx as torch computes them, bit for
    bit; dbias against float64 column sums; two runs, the same bits."""
    torch.manual_seed(R + C)
    x = torch.randn(R, C, device="cuda", requires_grad=True)
    b = torch.randn(C, device="cuda", requires_grad=True)
    g = torch.randn(R, C, device="cuda")
    y = ops.bias_lrelu(x, b, slope)
    gx, gb = torch.autograd.grad(y, [x, b], g, retain_graph=True)
    gx2, gb2 = torch.autograd.grad(y, [x, b], g)
    xr, br = x.detach().clone().requires_grad_(True), b.detach().clone().requires_grad_(True)
    yr = torch.nn.functional.leaky_relu(xr + br, slope)
    (gxr,) = torch.autograd.grad(yr, [xr], g)
    assert torch.equal(y, yr) and torch.equal(gx, gxr) and torch.equal(gx2, gxr)
    assert torch.equal(gb, gb2)
    check_err("ordered bias_lrelu dbias R=%d C=%d slope=%g vs float64" % (R, C, slope),
              rel_err(host(gb), f64(host(gxr)).sum(0)), DBIAS_BOUND)


@pytest.mark.parametrize("R,C,slope", BIAS_SHAPES)
def test_linear_bias_lrelu_ordered_bias_gradient(ops, R, C, slope):
    """The same launch behind the fused head layer: d = g * LeakyReLU'(y) from the saved output, dbias = the column sums
    of d against float64 (the mask read from the very output the layer saved), two runs, the same bits."""
    rng = np.random.default_rng(R + C)
    Kd = 16
    x = dev(rng.standard_normal((R, Kd)).astype(np.float32)).requires_grad_(True)
    W = dev((rng.standard_normal((C, Kd)) * 0.1).astype(np.float32)).requires_grad_(True)
    b = dev(rng.standard_normal(C).astype(np.float32)).requires_grad_(True)
    g = rng.standard_normal((R, C)).astype(np.float32)
    ops.step_begin()
    y = ops.linear_bias_lrelu(x, W, b, slope)
    runs = [torch.autograd.grad(y, [x, W, b], dev(g), retain_graph=True) for _ in range(2)]
    for a, c in zip(*runs):
        assert torch.equal(a, c)
    d = g * np.where(host(y) > 0, np.float32(1.0), np.float32(slope))
    check_err("ordered linear_bias_lrelu dbias R=%d C=%d slope=%g vs float64" % (R, C, slope),
              rel_err(host(runs[0][2]), f64(d).sum(0)), DBIAS_BOUND)


# ------------------------------------------------------------------------------------------------ e. serial regulariser

def test_regulariser_of_all_layers_in_one_workgroup_vs_float64(ops):
    """ops.deform_regularizer_all in deterministic mode (deform_regularizer_serial_kernel: one workgroup walks every
    layer and every block in order) on an empty layer, a layer with fewer valid rows than rows and an upstream factor
    other than 1: the value and every gradient against the float64 formula of the reference, zero gradient on the padded
    rows, the same bits in the loss from two runs."""
    torch.manual_seed(11)
    layers, leaves, n_valid = [], [], []
    for N, ext in ((300, 0.05), (64, 0.1), (0, 0.2), (1000, 0.2)):
        m = torch.rand(N, 15, device="cuda").requires_grad_(True)
        d = (torch.randn(N, 15, 3, device="cuda") * ext).requires_grad_(True)
        nv = torch.tensor([N - 7], dtype=torch.int32, device="cuda") if N == 300 else None
        layers.append((m, d, ext, 1.2, 1.0, nv))
        leaves += [m, d]
        n_valid.append(N - 7 if N == 300 else N)
    one = ops.deform_regularizer_all(layers)
    again = ops.deform_regularizer_all(layers)
    assert torch.equal(one, again)
    got = torch.autograd.grad(one * 0.37, leaves, allow_unused=True)
    want, want_grads = 0.0, []
    for (m, d, ext, rep, power, _), n in zip(layers, n_valid):
        if m.shape[0] == 0:
            want_grads += [None, None]
            continue
        term, m64, k64 = regulariser_float64(m, d, n, ext, rep, power)
        want_grads += list(torch.autograd.grad(term * 0.37, [m64, k64]))
        want = want + float(term.detach())
    check_err("ordered deform_regularizer_all value vs float64", abs(float(one.detach()) - want) / abs(want), REG_BOUND)
    for i, (a, w, n) in enumerate(zip(got, want_grads, np.repeat(n_valid, 2))):
        if w is None:
            assert a is None or a.numel() == 0
            continue
        check_err("ordered deform_regularizer_all gradient %d vs float64" % i, rel_err(host(a[:n]), host(w)), REG_BOUND)
        assert (a[n:] == 0).all()


# ------------------------------------------------------------------------------------------------ f. deform operands

@pytest.mark.parametrize("N,modulated", [(1, True), (257, True), (960, False), (5000, False)])
def test_deform_operands_backward_in_one_workgroup_vs_float64(ops, N, modulated):
    """mvk_deform_operands_bwd forced to one workgroup (deterministic mode: one ordered sum per column of d_bias): d_raw
    and d_bias against the reference's tensor expression (blocks.py:243-266, :287) in float64."""
    torch.manual_seed(N)
    K, ext = 15, 0.048
    D = (4 if modulated else 3) * K
    raw = torch.randn(N, D, device="cuda", requires_grad=True)
    bias = torch.randn(D, device="cuda", requires_grad=True)
    kp = torch.randn(K, 3, device="cuda")
    go, gd, gf, gm = (torch.randn(*s, device="cuda") for s in ((N, K, 3), (N, K, 3), (N, D), (N, K)))
    ops.step_begin()
    feat, off, dkp, mod = ops.deform_operands(raw, bias, kp, ext, modulated)
    loss = (off * go).sum() + (dkp * gd).sum() + (feat * gf).sum()
    if modulated:
        loss = loss + (mod * gm).sum()
    g_raw, g_bias = torch.autograd.grad(loss, [raw, bias])
    r2, b2 = raw.detach().double().requires_grad_(True), bias.detach().double().requires_grad_(True)
    f2 = r2 + b2
    o2 = f2[:, :3 * K].reshape(-1, K, 3) * ext
    l2 = (o2 * go.double()).sum() + ((o2 + kp.double()) * gd.double()).sum() + (f2 * gf.double()).sum()
    if modulated:
        l2 = l2 + (2 * torch.sigmoid(f2[:, 3 * K:]) * gm.double()).sum()
    w_raw, w_bias = torch.autograd.grad(l2, [r2, b2])
    label = "ordered deform_operands N=%d modulated=%d " % (N, modulated)
    check_err(label + "d_raw vs float64", rel_err(host(g_raw), host(w_raw)), D_RAW_BOUND)
    check_err(label + "d_bias vs float64", rel_err(host(g_bias), host(w_bias)), DBIAS_BOUND)


# ------------------------------------------------------------------------------------------------ g. elementwise

@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_add_lrelu_equals_torch(ops, n):
    """mvk_add_lrelu_fwd/bwd: LeakyReLU(a + b) and both gradients bit for bit, sums that are exactly zero and negative sums
    included; the two gradients are distinct tensors (downstream nodes accumulate onto theirs in place)."""
    rng = np.random.default_rng(n)
    a = rng.standard_normal(n).astype(np.float32)
    b = rng.standard_normal(n).astype(np.float32)
    b[::3] = -a[::3]                                                  # a + b == 0 exactly
    b[1::3] = -np.abs(b[1::3]) - np.abs(a[1::3])                      # a + b < 0
    assert ((a + b) == 0).any() and ((a + b) < 0).any() == (n > 1)
    g = dev(rng.standard_normal(n).astype(np.float32))
    at, bt = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    ar, br = dev(a).requires_grad_(True), dev(b).requires_grad_(True)
    y = ops.add_lrelu(at, bt, 0.1)
    yr = torch.nn.functional.leaky_relu(ar + br, 0.1)
    assert bits_equal(host(y), host(yr))
    ga, gb = torch.autograd.grad(y, [at, bt], g)
    gar, gbr = torch.autograd.grad(yr, [ar, br], g)
    assert bits_equal(host(ga), host(gar)) and bits_equal(host(gb), host(gbr))
    assert ga.data_ptr() != gb.data_ptr()


@pytest.mark.parametrize("shape", [(1, 4, 3, 5), (2, 64, 5, 7), (1, 68, 3, 11), (3, 4, 17, 21)])
def test_bias_act_nhwc_equals_the_torch_expression(ops, shape):
    """mvk_bias_act_nhwc: act(x + bias[c] (+ res (+ bias2[c]))) over channels-last tensors whose float4 count is no
    multiple of the workgroup, every combination of residual / second bias / ReLU, in place and into `out`."""
    torch.manual_seed(shape[1] + shape[3])
    assert (np.prod(shape) // 4) % 256 != 0

    def nhwc():
        return torch.randn(*shape, device="cuda").contiguous(memory_format=torch.channels_last)

    x, res = nhwc(), nhwc()
    bias, bias2 = torch.randn(shape[1], device="cuda"), torch.randn(shape[1], device="cuda")
    for with_res, with_b2, relu in itertools.product((False, True), (False, True), (False, True)):
        if with_b2 and not with_res:
            continue
        want = x + bias[None, :, None, None]
        if with_res:
            want = want + res
        if with_b2:
            want = want + bias2[None, :, None, None]
        if relu:
            want = torch.relu(want)
        args = (bias, res if with_res else None, bias2 if with_b2 else None, relu)
        mine = x.clone(memory_format=torch.preserve_format)
        got = ops.bias_act_nhwc(mine, *args)
        assert got is mine and bits_equal(host(got), host(want)), args[1:]
        out = torch.full_like(x, 7.0)
        src = x.clone(memory_format=torch.preserve_format)
        assert ops.bias_act_nhwc(src, *args, out=out) is out
        assert bits_equal(host(out), host(want)) and torch.equal(src, x)
    with pytest.raises(RuntimeError):
        ops.bias_act_nhwc(x.clone(memory_format=torch.preserve_format), bias, None, bias2)          # a second bias needs a residual


def test_bias_act_nhwc_refuses_channels_that_are_no_multiple_of_four(ops):
    x = torch.randn(2, 6, 3, 5, device="cuda").contiguous(memory_format=torch.channels_last)
    with pytest.raises(RuntimeError):
        ops.bias_act_nhwc(x, torch.randn(6, device="cuda"))
