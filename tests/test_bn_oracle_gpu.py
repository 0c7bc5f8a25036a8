"""GPU: the masked BatchNorm + LeakyReLU kernels of csrc/bn.hip against the float64 oracle of tests/bn_ref.py, every
channel of every tensor under the referee rule err_c(HIP, f64) <= REFEREE_FACTOR * err_c(float32 tensor expression on
the same device, f64) + REFEREE_FLOOR (tests/util.py), gradients included. Own-statistics families (one workgroup per
64 channels, register-resident rows, two-stage) over bn_ref.CASES; then the hot path of the big levels, where the
statistics arrive as (sum, centred M2) partials from the producing product's epilogue (bn_sum_partials_m2) and the
backward runs on the mean / invstd that merge saved -- there the BatchNorm's input is the float32 product as the HIP
path wrote it, so only the BatchNorm is judged. Scope and exclusions: the docstring of tests/bn_ref.py."""
import numpy as np
import pytest
import torch

import bn_ref as ref
from util import bits_equal

pytestmark = pytest.mark.gpu

IDS = [ref.case_id(c) for c in ref.CASES]


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import mvkpconv
    return mvkpconv.sub("ops")


def dev(a, misaligned=False):
    """a on the device; misaligned: contiguous, its storage starting one float past a 16-byte boundary."""
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    if not misaligned:
        return t
    buf = torch.empty(t.numel() + 1, device="cuda", dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4 and v.is_contiguous()
    return v


def host(t):
    return t.detach().cpu().numpy()


def module(D, gamma, beta, momentum):
    bn = torch.nn.BatchNorm1d(D, momentum=momentum).cuda()
    with torch.no_grad():
        bn.weight.copy_(gamma)
        bn.bias.copy_(beta)
    return bn


def run_hip(ops, x, n, gamma, beta, slope, addend, go):
    """ops.bn_lrelu on device tensors (x a leaf that requires grad and may carry producer statistics). The batch mean
    and variance read back through the running statistics of a fresh module (running_mean = running_var = 0,
    momentum = 1: the update is then the statistic itself); after that two identical calls of the module under test
    (momentum 0.02) with their backwards. Returns (the dict bn_ref.compare takes with full-height 2-D tensors, the
    first call's (y, dx, dgamma, dbeta), the batch counter)."""
    D = x.shape[1]
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    probe = module(D, gamma, beta, 1.0)
    with torch.no_grad():
        probe.running_var.zero_()
        ops.bn_lrelu(x, nv, probe, slope=slope, addend=addend)
    bn = module(D, gamma, beta, ref.MOMENTUM)
    leaves = [x, bn.weight, bn.bias] + ([addend] if addend is not None else [])
    calls = []
    for _ in range(2):
        y = ops.bn_lrelu(x, nv, bn, slope=slope, addend=addend)
        gx, gw, gb, *gs = torch.autograd.grad(y, leaves, go)
        calls.append((host(y), host(gx), host(gw), host(gb)))
    unbiased = host(probe.running_var).astype(np.float64)
    out = {"y": calls[1][0], "dx": calls[1][1], "dgamma": calls[1][2], "dbeta": calls[1][3],
           "d_addend": host(gs[0]) if gs else None, "mean": host(probe.running_mean),
           "var": unbiased * ((n - 1.0) / n) if n > 1 else unbiased,
           "running_mean": host(bn.running_mean), "running_var": host(bn.running_var)}
    return out, calls[0], int(bn.num_batches_tracked)


def check_run(label, out, first, counter, n, ref32, oracle_of):
    """What every run must show: padded rows exactly zero, two batches counted, the second identical forward and
    backward bit-equal to the first (BatchNorm partials are combined in a fixed order), and every tensor
    inside the referee bound in every channel."""
    for name in ("y", "dx", "d_addend"):
        assert out[name] is None or not out[name][n:].any(), name
    assert counter == 2
    for a, b, name in zip(first, (out["y"], out["dx"], out["dgamma"], out["dbeta"]), ("y", "dx", "dgamma", "dbeta")):
        assert bits_equal(a, b), name
    ref.compare(label, out, ref32, oracle_of)


@pytest.mark.parametrize("c", ref.CASES, ids=IDS)
def test_own_statistics_families_vs_float64_oracle(ops, c):
    """Every case of bn_ref.CASES through ops.bn_lrelu (the case's family is the one csrc/bn.hip dispatches it to)."""
    inp = ref.inputs(c)
    mis = c.variant == "misaligned"
    assert ops.bn_single_launch_rows(c.D) == (1024 if c.D % 4 == 0 else 128)      # the families the table is laid out for
    assert (c.family == "small") == (c.R <= 128)
    assert (c.family == "mid") == (128 < c.R <= ops.bn_single_launch_rows(c.D) and not mis)
    x = dev(inp["x"], mis).requires_grad_(True)
    addend = dev(inp["addend"], mis).requires_grad_(True) if c.join else None
    out, first, counter = run_hip(ops, x, c.n, dev(inp["gamma"]), dev(inp["beta"]), c.slope, addend, dev(inp["go"], mis))
    check_run("bn " + ref.case_id(c), out, first, counter, c.n, ref.ref32_of_case(c, inp, "cuda"), ref.oracle_of_case(c, inp))


def _judge_product(ops, label, y_lin, st, n, join, seed):
    """The BatchNorm behind a product whose epilogue wrote the statistics partials st = (partials, rows per block):
    forward and backward against the oracle of the float32 product itself."""
    M, N = y_lin.shape
    rng = np.random.default_rng(seed)
    f = np.float32
    gamma, beta = rng.uniform(0.5, 1.5, N).astype(f), rng.uniform(-0.5, 0.5, N).astype(f)
    go = rng.standard_normal((M, N)).astype(f)
    ad = rng.standard_normal((M, N)).astype(f) if join else None
    assert st is not None and st[0].shape == ((M + st[1] - 1) // st[1], 2, N)
    x = y_lin.detach()
    x._mvk_bn_stats = st
    x.requires_grad_(True)
    addend = dev(ad).requires_grad_(True) if join else None
    out, first, counter = run_hip(ops, x, n, dev(gamma), dev(beta), 0.1, addend, dev(go))
    xh = host(y_lin)
    run0 = ref.RUNNING0(N)
    oracle_of = lambda y: ref.oracle(xh, n, gamma, beta, ref.EPS, 0.1, ad, go, y, run0, ref.MOMENTUM, 2)
    r32 = ref.ref32(xh, n, gamma, beta, ref.EPS, 0.1, ad, go, run0, ref.MOMENTUM, 2, "cuda")
    check_run(label, out, first, counter, n, r32, oracle_of)


@pytest.mark.parametrize("M,N,K,n,join,edge", [(1300, 64, 32, 1207, False, "idle_lanes"), (1300, 64, 32, 1207, True, "idle_lanes"),
                                               (4200, 64, 48, 4100, False, "four_per_trip"), (300, 66, 32, 263, False, None)])
def test_tiled_product_partials_forward_and_backward_vs_float64_oracle(ops, M, N, K, n, join, edge):
    """ops.gemm(..., split_k=1, stats_n_valid=) hands (sum, centred M2) per row block to the BatchNorm: 1300 rows leave
    some of the 16 reducing lanes of bn_sum_partials_m2 idle (or end on a ragged block), 4200 rows with column means
    more than ten sigma away run its four-blocks-per-trip loop, 300 x 66 is the shape that emits statistics above 128 rows
    because N % 4 != 0."""
    rng = np.random.default_rng(M + N + K)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    if edge == "four_per_trip":
        A[:, 0] = 40.0                                 # a large common component: column means up to 13 sigma away
    A, B = dev(A), dev(B)
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    y_lin, st = ops.gemm(A, B, split_k=1, stats_n_valid=nv)
    assert st is not None, "this shape must carry epilogue statistics"
    rows = st[1]
    blocks = (n + rows - 1) // rows                    # row blocks that hold valid rows
    if edge == "idle_lanes":
        assert blocks < 16 or n % rows != 0, (rows, blocks)
    if edge == "four_per_trip":
        assert blocks > 48, (rows, blocks)
        mu, sd = y_lin[:n].mean(0), y_lin[:n].std(0)
        assert (mu.abs() / sd).max().item() > 10
    _judge_product(ops, "bn after tiled product %dx%dx%d n=%d%s" % (M, N, K, n, " join" if join else ""), y_lin, st, n, join,
                   M + N)


def test_streaming_product_partials_forward_and_backward_vs_float64_oracle(ops, monkeypatch):
    """The same behind the streaming f32 contraction (csrc/gemm32s.hip), whose row blocks are 16 x tiles rows."""
    M, N, K, n = 4100, 64, 30, 4063
    monkeypatch.setenv("MVK_GEMM32_STREAM", "2")
    ok, tiles, wgs, need = ops.gemm_f32_stream_plan(M, N, K)
    assert ok and need == 0
    rng = np.random.default_rng(M + N + K)
    A, W = dev(rng.standard_normal((M, K)).astype(np.float32)), dev((rng.standard_normal((K, N)) * 0.2).astype(np.float32))
    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
    y_lin, st = ops.gemm_f32_stream(A, W, nv)
    assert st[1] == 16 * tiles and st[0].shape == (wgs, 2, N)
    _judge_product(ops, "bn after streaming product %dx%dx%d n=%d" % (M, N, K, n), y_lin, st, n, False, M + N)
