"""GPU: every fused product of csrc/gemm.hip against the int64 / float64 oracle of tests/gemm_ref.py.

Family I (integers in [-4, 4]: float32 arithmetic is exact in any order) is compared BIT FOR BIT; Family R (plain
products) per element against (K + 4) 2^-24 (|A|.|B|)_ij; the centred squares of the statistics epilogue against the
bound derived in gemm_ref.m2_bound. Every expected value comes from gemm_ref.py; no launch is compared with another
launch, except the stated bit-reproducibility repeats of the ordered mode.

Operands live as contiguous views inside NaN-filled buffers, a NaN band before and after each, 0 / 1 / 2 floats off a
16-byte boundary: a read outside an operand or a masked lane that leaks shows as NaN in the output. Where an entry point
takes out=, the output is a NaN-prefilled view inside such a buffer; its bands must still be NaN afterwards. Everything
runs in default mode (f32 atomics for split reductions) and in ordered mode (ops.set_deterministic).

OUT OF SCOPE, with the reason:
  * the operand transform and finished statistics (mvk_gemm_f32_bn, mvk_gemm_f32_pair_bn): off by default, owned by
    tests/test_bn_fold_gpu.py;
  * the streaming kernel of csrc/gemm32s.hip: not planned below 4 096 rows, has its own float64 test;
  * graph capture of the grouped launch: test_deferred_weight_gradients_run_as_one_grouped_launch (tests/test_gpu_parity.py)
    covers it.
"""
import contextlib

import numpy as np
import pytest
import torch

import gemm_ref as ref
from util import bits_equal, check_err

pytestmark = pytest.mark.gpu

BAND = 64
MODES = ("default", "ordered")


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    import mvkpconv
    return mvkpconv.sub("ops")


@contextlib.contextmanager
def in_mode(ops, name):
    """Default (atomic) or ordered split reductions; in ordered mode a scatter without a reverse list raises instead of
    silently taking the atomic path."""
    def refuse(what):
        raise AssertionError("ordered mode found no reverse list for %s" % what)

    was = ops.is_deterministic()
    patch = pytest.MonkeyPatch()
    ops.set_deterministic(name == "ordered")
    try:
        assert ops.is_deterministic() == (name == "ordered") and ops.lib().mvk_gemm_split_ordered() == int(name == "ordered")
        patch.setattr(ops, "_no_reverse_list", refuse)
        yield
    finally:
        patch.undo()
        ops.set_deterministic(was)


class Pack:
    """float32 arrays as views of ONE NaN-filled device buffer: BAND NaNs around each, `off` floats past a 16-byte
    boundary. One upload, one download."""

    def __init__(self):
        self.items, self.n, self.dev, self.views = [], 0, None, None

    def add(self, a, off=0):
        a = np.ascontiguousarray(a, np.float32)
        start = (self.n + BAND + 3) // 4 * 4 + off
        self.items.append((start, a))
        self.n = start + a.size
        return len(self.items) - 1

    def upload(self):
        h = np.full((self.n + BAND + 3) // 4 * 4, np.nan, np.float32)
        for s, a in self.items:
            h[s:s + a.size] = a.ravel()
        self.dev = torch.from_numpy(h).cuda()
        assert self.dev.data_ptr() % 16 == 0
        self.views = [self.dev[s:s + a.size].view(a.shape) for s, a in self.items]
        for (s, _), v in zip(self.items, self.views):
            assert v.is_contiguous() and v.data_ptr() % 16 == 4 * (s % 4)
        return self.views

    def download(self):
        """The views' contents; everything between them must still be NaN."""
        h = self.dev.cpu().numpy()
        inside = np.zeros(h.shape, bool)
        out = []
        for s, a in self.items:
            inside[s:s + a.size] = True
            out.append(h[s:s + a.size].reshape(a.shape))
        assert np.isnan(h[~inside]).all(), "a guard band was written"
        return out


def fetch(tensors):
    """Device tensors -> NumPy arrays with one copy."""
    ts = [t.detach() for t in tensors]
    flat = torch.cat([t.reshape(-1).float() for t in ts]).cpu().numpy() if ts else np.zeros(0, np.float32)
    out, o = [], 0
    for t in ts:
        out.append(flat[o:o + t.numel()].reshape(tuple(t.shape)))
        o += t.numel()
    return out


def force_env(monkeypatch, force):
    if force is None:
        monkeypatch.delenv("MVK_GEMM_FORCE", raising=False)
    else:
        monkeypatch.setenv("MVK_GEMM_FORCE", "%d,%d,%d" % tuple(force))


# ------------------------------------------------------------------------------------------ a. plain product

def run_plain(ops, cases, monkeypatch, runs=1):
    """Every case through ops.gemm(out=guarded view) `runs` times on fresh outputs -> per run the list of outputs."""
    ins, outs = Pack(), [Pack() for _ in range(runs)]
    for i, c in enumerate(cases):
        A, B, base = ref.operands(c)
        ins.add(A, c.offA)
        ins.add(B, c.offB)
        for o in outs:
            o.add(base if base is not None else np.full((c.M, c.N), np.nan, np.float32), i % 3)
    v = ins.upload()
    for o in outs:
        o.upload()
        for i, c in enumerate(cases):
            A, B, dst = v[2 * i], v[2 * i + 1], o.views[i]
            assert A.data_ptr() % 16 == 4 * c.offA and B.data_ptr() % 16 == 4 * c.offB
            force_env(monkeypatch, c.force)
            r = ops.gemm(A, B, transA=c.layout[0] == "T", transB=c.layout[1] == "T", out=dst, accumulate=c.accumulate)
            assert r.data_ptr() == dst.data_ptr()
    torch.cuda.synchronize()
    return [o.download() for o in outs]


def judge_plain(label, cases, got):
    worst = 0.0
    for c, g in zip(cases, got):
        A, B, base = ref.operands(c)
        want = ref.product(A, B, c.layout, base)
        if c.family == "I":
            assert ref.exact(g, want), "%s %s: not the exact product" % (label, ref.case_id(c))
        else:
            ratio = ref.r_ratio(g, want, ref.abs_product(A, B, c.layout), c.K)
            assert ratio <= 1.0, "%s %s: err / bound = %.3g" % (label, ref.case_id(c), ratio)
            worst = max(worst, ratio)
    if any(c.family == "R" for c in cases):
        check_err("gemm oracle %s: Family R, largest err / ((K + 4) 2^-24 |A|.|B|)" % label, worst, 1.0)


@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_plain_product_every_path_and_plan_default_mode(ops, layout, monkeypatch):
    """PLAIN_CASES of one layout: every loader pipeline x k-tile count x tail, every forced plan x split, every tile edge,
    every vector width, accumulate onto an integer base; split reductions add with f32 atomics."""
    cases = [c for c in ref.PLAIN_CASES if c.layout == layout]
    with in_mode(ops, "default"):
        (got,) = run_plain(ops, cases, monkeypatch)
    judge_plain("plain %s default" % layout, cases, got)


@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_plain_product_split_cases_ordered_mode_twice_the_same_bits(ops, layout, monkeypatch):
    """The cases that ask for a split, under the ordered reduction: exact / inside the bound, and two runs bit-identical."""
    cases = [c for c in ref.PLAIN_CASES if c.layout == layout and c.force[2] > 1]
    assert len(cases) >= 18
    with in_mode(ops, "ordered"):
        first, second = run_plain(ops, cases, monkeypatch, runs=2)
    judge_plain("plain %s ordered" % layout, cases, first)
    for c, a, b in zip(cases, first, second):
        assert bits_equal(a, b), ref.case_id(c)


# ------------------------------------------------------------------------------------------ b. out= without accumulate

@pytest.mark.parametrize("layout", ref.LAYOUTS)
def test_out_without_accumulate_is_the_product_when_the_plan_splits(ops, layout, monkeypatch):
    """ops.gemm(A, B, out=X) on a shape whose OWN plan splits (small M, deep K), default mode, X NaN-prefilled: X must be
    the exact product, not X_old + A.B (the atomic split adds onto its output)."""
    force_env(monkeypatch, None)
    c = ref.Case(layout, 20, 64, 1024, 0, 0, (0, 0, 0), "I", False)
    A, B, _ = ref.operands(c)
    ins, out = Pack(), Pack()
    ins.add(A), ins.add(B), out.add(np.full((c.M, c.N), np.nan, np.float32), 1)
    a, b = ins.upload()
    (dst,) = out.upload()
    with in_mode(ops, "default"):
        assert ops.gemm_plan(c.M, c.N, c.K)[0] > 1, "this shape was chosen because its plan splits"
        ops.gemm(a, b, transA=layout[0] == "T", transB=layout[1] == "T", out=dst)
        seven = torch.full((c.M, c.N), 7.0, device="cuda")
        ops.gemm(a, b, transA=layout[0] == "T", transB=layout[1] == "T", out=seven)
    want = ref.product(A, B, layout)
    assert ref.exact(out.download()[0], want)
    assert ref.exact(fetch([seven])[0], want)


# ------------------------------------------------------------------------------------------ c. linear_bias_lrelu

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("slope", ref.BIAS_SLOPES)
def test_linear_bias_lrelu_forward_and_three_gradients(ops, slope, mode, monkeypatch):
    force_env(monkeypatch, None)
    ins = Pack()
    for i, s in enumerate(ref.BIAS_SHAPES):
        x, W, b, g = ref.bias_inputs(*s)
        ins.add(x, i % 3), ins.add(W, (i // 3) % 3), ins.add(b, (i + 1) % 3), ins.add(g, (i + 2) % 3)
    v = ins.upload()
    res = []
    with in_mode(ops, mode):
        for i in range(len(ref.BIAS_SHAPES)):
            x, W, b, g = v[4 * i:4 * i + 4]
            x.requires_grad_(True), W.requires_grad_(True), b.requires_grad_(True)
            y = ops.linear_bias_lrelu(x, W, b, slope)
            res += [y] + list(torch.autograd.grad(y, [x, W, b], g))
        res = fetch(res)
    for i, s in enumerate(ref.BIAS_SHAPES):
        r = ref.linear_bias_lrelu(*ref.bias_inputs(*s)[:3], slope, ref.bias_inputs(*s)[3])
        assert (r["pre"] == 0).any() and (r["pre"] < 0).any()
        for name, got in zip(("y", "dx", "dW", "db"), res[4 * i:4 * i + 4]):
            assert ref.exact(got, r[name]), (s, slope, name)


# ------------------------------------------------------------------------------------------ d. linear_pair

def judge_partials(label, st, want_product, n_valid, exact_sums=True):
    """(partials, rows) of a statistics epilogue against the float64 partials of `want_product`: exact column sums
    (Family I), (0, 0) beyond n_valid, centred squares inside gemm_ref.m2_bound. Returns the largest err / bound."""
    part, rows = st
    sums, m2, cnt = ref.stats_partials(want_product, n_valid, rows)
    assert part.shape == (sums.shape[0], 2, sums.shape[1]), label
    part = part.astype(np.float64)
    assert np.isfinite(part).all(), label
    if exact_sums:
        assert np.array_equal(part[:, 0], sums), label + ": column sums"
    dead = cnt == 0
    assert not part[dead].any(), label + ": a block beyond n_valid must give (0, 0)"
    bound = ref.m2_bound(m2, sums, cnt, rows)
    err = np.abs(part[:, 1] - m2)
    assert (err <= bound).all(), "%s: centred squares off by %.3g x the bound" % (label, (err / np.maximum(bound, 1e-300)).max())
    live = bound > 0
    return float((err[live] / bound[live]).max()) if live.any() else 0.0


@pytest.mark.parametrize("mode", MODES)
def test_linear_pair_outputs_partials_and_gradients(ops, mode, monkeypatch):
    force_env(monkeypatch, None)
    worst = 0.0
    with in_mode(ops, mode):
        M, N0, N1, Kd = ref.PAIR_NONE
        x, W0, W1, _, _ = (torch.from_numpy(t).cuda() for t in ref.pair_inputs(M, N0, N1, Kd))
        assert ops.linear_pair(x, W0, W1) is None, "a narrow partner with Kd > 512 cannot ride the wide tiles"
        for ci, (M, N0, N1, Kd, stats) in enumerate(ref.PAIR_CASES):
            inp = ref.pair_inputs(M, N0, N1, Kd)
            ins = Pack()
            for j, t in enumerate(inp):
                ins.add(t, (ci + j) % 3)
            x, W0, W1, g0, g1 = ins.upload()
            n = M - 7
            nv = torch.tensor([n], dtype=torch.int32, device="cuda") if stats else None
            x.requires_grad_(True), W0.requires_grad_(True), W1.requires_grad_(True)
            pair = ops.linear_pair(x, W0, W1, nv)
            assert pair is not None, (M, N0, N1, Kd)
            y0, y1 = pair
            grads = torch.autograd.grad([y0, y1], [x, W0, W1], [g0, g1])
            sts = [ops.bn_stats_of(y) for y in (y0, y1)]
            assert all((st is not None) == stats for st in sts), (M, N0, N1, Kd, stats)
            got = fetch([y0, y1] + list(grads) + [st.partials for st in sts if st is not None])
            r = ref.linear_pair(*inp)
            for name, g in zip(("y0", "y1", "dx", "dW0", "dW1"), got):
                assert ref.exact(g, r[name]), (M, N0, N1, Kd, name)
            if stats:
                for k, st in enumerate(sts):
                    worst = max(worst, judge_partials("pair %s output %d" % ((M, N0, N1, Kd), k), (got[5 + k], st.rows),
                                                      r["y%d" % k], n))
    check_err("gemm oracle pair %s: centred squares, largest err / bound" % mode, worst, 1.0)


# ------------------------------------------------------------------------------------------ e. gemm_dual

@pytest.mark.parametrize("mode", MODES)
def test_gemm_dual_at_every_split_of_the_concatenated_reduction(ops, mode, monkeypatch):
    with in_mode(ops, mode):
        force_env(monkeypatch, None)
        for c in ref.DUAL_NONE:
            assert ops.gemm_dual(*(torch.from_numpy(t).cuda() for t in ref.dual_inputs(*c))) is None, c
        res, wants = [], []
        for ci, c in enumerate(ref.DUAL_CASES):
            inp = ref.dual_inputs(*c)
            ins = Pack()
            for j, t in enumerate(inp):
                ins.add(t, (ci + j) % 3)
            v = ins.upload()
            ksteps = ref.cdiv(c[2] + c[3], ref.BK)
            for s in range(1, ksteps + 2):                     # ksteps + 1: more splits asked than there are k-tiles
                force_env(monkeypatch, (0, 0, s))
                out = ops.gemm_dual(*v)
                assert out is not None, (c, s)
                res.append(out)
                wants.append((c, s, ref.gemm_dual(*inp)))
        res = fetch(res)
    for got, (c, s, want) in zip(res, wants):
        assert ref.exact(got, want), (c, s)


# ------------------------------------------------------------------------------------------ f. upsample_cat_linear

@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("idt", [torch.int32, torch.int64])
def test_upsample_cat_linear_output_and_three_gradients(ops, idt, mode, monkeypatch):
    force_env(monkeypatch, None)
    res, wants = [], []
    with in_mode(ops, mode):
        for ci, c in enumerate(ref.UPCAT_CASES):
            Ns = c[0]
            for kind in ref.UPCAT_INDEX_KINDS:
                xh, idx, sh, Wh, gh = ref.upcat_inputs(*c, kind)
                ins = Pack()
                for j, t in enumerate((xh, sh, Wh, gh)):
                    ins.add(t, (ci + j) % 3)
                x, skip, W, g = ins.upload()
                inds = torch.from_numpy(idx).to(idt).cuda()
                if mode == "ordered":
                    ops.remember_reverse(inds, ops.reverse_neighbors(inds, Ns, first_column=True), first_column=True)
                x.requires_grad_(True), skip.requires_grad_(True), W.requires_grad_(True)
                y = ops.upsample_cat_linear(x, inds, skip, W)
                first = torch.autograd.grad(y, [x, skip, W], g, retain_graph=True)
                second = torch.autograd.grad(y, [x, skip, W], g)
                for a, b in zip(first, second):
                    assert torch.equal(a, b), "a second backward on the same graph must give the same bits"
                res += [y] + list(first)
                wants.append((c, kind, ref.upsample_cat_linear(xh, idx, sh, Wh, gh)))
        res = fetch(res)
    for i, (c, kind, r) in enumerate(wants):
        for name, got in zip(("y", "dx", "dskip", "dW"), res[4 * i:4 * i + 4]):
            assert ref.exact(got, r[name]), (c, kind, name)


# ------------------------------------------------------------------------------------------ g. kp_transposed_contraction

@pytest.mark.parametrize("mode", MODES)
def test_kp_transposed_contraction_and_its_fallback(ops, mode, monkeypatch):
    force_env(monkeypatch, None)
    res = []
    with in_mode(ops, mode):
        for ci, c in enumerate(ref.KP_CASES):
            ins = Pack()
            A2, W = ref.kp_inputs(*c)
            ins.add(A2, ci % 3), ins.add(W, (ci + 1) % 3)
            res.append(ops.kp_transposed_contraction(*ins.upload()))
        res = fetch(res)
    for c, got in zip(ref.KP_CASES, res):
        assert ref.exact(got, ref.kp_transposed_contraction(*ref.kp_inputs(*c))), c


# ------------------------------------------------------------------------------------------ h. gemm_ldb

@pytest.mark.parametrize("mode", MODES)
def test_gemm_ldb_reads_only_its_column_block(ops, mode, monkeypatch):
    res = []
    with in_mode(ops, mode):
        for ci, (M, Kd, col0, N, ldb, split) in enumerate(ref.LDB_CASES):
            A, Bw = ref.ldb_inputs(M, Kd, ldb)
            Bn = Bw.copy()
            Bn[:, :col0] = np.nan
            Bn[:, col0 + N:] = np.nan                          # the neighbouring columns of the wide matrix
            ins = Pack()
            ins.add(A, ci % 3), ins.add(Bn, (ci // 3) % 3)
            a, b = ins.upload()
            force_env(monkeypatch, (0, 0, split) if split else None)
            res.append(ops.gemm_ldb(a, b, col0, N, ldb))
        res = fetch(res)
    for (M, Kd, col0, N, ldb, split), got in zip(ref.LDB_CASES, res):
        A, Bw = ref.ldb_inputs(M, Kd, ldb)
        assert ref.exact(got, ref.gemm_ldb(A, Bw, col0, N)), (M, Kd, col0, N, ldb, split)


# ------------------------------------------------------------------------------------------ i. statistics epilogue

def stats_cases(mode):
    return [c for c in ref.STATS_CASES if c[3] == 1 or mode == "ordered"]


def n_valids(M, block=64):
    return (0, 1, block - 1, block, block + 1, M)


@pytest.mark.parametrize("mode", MODES)
def test_statistics_epilogue_sums_exact_and_centred_squares_bounded(ops, mode, monkeypatch):
    """Family I: the product and the column sums of every row block exact, (0, 0) for blocks beyond n_valid, the centred
    squares inside the derived bound; unsplit in both modes, split under the ordered reduction. Normal data with a
    constant-40 column (means far from zero): the product per element inside the Family-R bound, the centred squares
    against the float64 partials of the float32 product as the launch wrote it (the epilogue's own input)."""
    force_env(monkeypatch, None)
    worst = {"I": 0.0, "N": 0.0, "Nprod": 0.0}
    with in_mode(ops, mode):
        for (M, N, K, split) in stats_cases(mode):
            assert M > ops.bn_single_launch_rows(N)
            for fam in ("I", "N"):
                Ah, Bh = ref.stats_inputs(M, N, K, fam)
                ins = Pack()
                ins.add(Ah), ins.add(Bh)
                A, B = ins.upload()
                res, rows = [], None
                for n in n_valids(M):
                    nv = torch.tensor([n], dtype=torch.int32, device="cuda")
                    y, st = ops.gemm(A, B, split_k=split, stats_n_valid=nv)
                    assert st is not None and st[1] == 64, (M, N, K, split)
                    rows = st[1]
                    res += [y, st[0]]
                res = fetch(res)
                want = ref.product(Ah, Bh)
                for k, n in enumerate(n_valids(M)):
                    y, part = res[2 * k], res[2 * k + 1]
                    label = "stats %s %s n_valid=%d %s" % ((M, N, K, split), fam, n, mode)
                    if fam == "I":
                        assert ref.exact(y, want), label
                        worst["I"] = max(worst["I"], judge_partials(label, (part, rows), want, n))
                    else:
                        ratio = ref.r_ratio(y, want, ref.abs_product(Ah, Bh), K)
                        assert ratio <= 1.0, label
                        worst["Nprod"] = max(worst["Nprod"], ratio)
                        worst["N"] = max(worst["N"], judge_partials(label, (part, rows), y, n, exact_sums=False))
    check_err("gemm oracle statistics %s: integer data, centred squares err / bound" % mode, worst["I"], 1.0)
    check_err("gemm oracle statistics %s: normal data, centred squares err / bound" % mode, worst["N"], 1.0)
    check_err("gemm oracle statistics %s: normal data, product err / ((K + 4) 2^-24 |A|.|B|)" % mode, worst["Nprod"], 1.0)


@pytest.mark.parametrize("mode", MODES)
def test_batchnorm_fed_the_epilogue_partials_meets_the_float64_oracle(ops, mode, monkeypatch):
    """ops.bn_lrelu on these partials against bn_ref's float64 BatchNorm of the float32 product, under the referee rule
    of tests/test_bn_oracle_gpu.py (whose judge is used as it stands)."""
    import test_bn_oracle_gpu as bn_oracle
    force_env(monkeypatch, None)
    with in_mode(ops, mode):
        for (M, N, K, split) in stats_cases(mode):
            Ah, Bh = ref.stats_inputs(M, N, K, "N")
            A, B = torch.from_numpy(Ah).cuda(), torch.from_numpy(Bh).cuda()
            for n in (65, M):
                nv = torch.tensor([n], dtype=torch.int32, device="cuda")
                y, st = ops.gemm(A, B, split_k=split, stats_n_valid=nv)
                bn_oracle._judge_product(ops, "gemm oracle bn after %dx%dx%d split %d n=%d %s" % (M, N, K, split, n, mode), y, st, n,
                                         False, M + N + n)


# ------------------------------------------------------------------------------------------ j. grouped weight gradients

@pytest.mark.parametrize("mode", MODES)
def test_grouped_weight_gradients_exact(ops, mode, monkeypatch):
    """ops._dw_gemm inside ops.defer_weight_grads(): wide and narrow outputs, reductions of 1 .. 1100 rows, heights of
    1 .. 70 in ONE grouped launch, and the N <= 16 product that is computed at once."""
    force_env(monkeypatch, None)
    cases = ref.DW_CASES
    ins = Pack()
    for i, c in enumerate(cases + [ref.DW_SMALL]):
        A, B = ref.dw_inputs(*c)
        ins.add(A, i % 3), ins.add(B, (i // 3) % 3)
    v = ins.upload()
    with in_mode(ops, mode):
        with ops.defer_weight_grads():
            outs = [ops._dw_gemm(v[2 * i], v[2 * i + 1]) for i in range(len(cases))]
            small = ops._dw_gemm(v[-2], v[-1])
        res = fetch(outs + [small])
    for c, got in zip(cases + [ref.DW_SMALL], res):
        assert got.shape == (c[1], c[2])
        assert ref.exact(got, ref.product(*ref.dw_inputs(*c), "TN")), c


# ------------------------------------------------------------------------------------------ k. linear(passthrough=True)

@pytest.mark.parametrize("mode", MODES)
def test_linear_passthrough_gradients_with_and_without_the_alias(ops, mode, monkeypatch):
    force_env(monkeypatch, None)
    res, wants = [], []
    with in_mode(ops, mode):
        for ci, c in enumerate(ref.PASS_CASES):
            inp = ref.pass_inputs(*c)
            for use_alias in (False, True):
                ins = Pack()
                for j, t in enumerate(inp):
                    ins.add(t, (ci + j) % 3)
                x, W, g, ga = ins.upload()
                x.requires_grad_(True), W.requires_grad_(True)
                y, alias = ops.linear(x, W, passthrough=True)
                if use_alias:      # (the backward may add g W onto the alias' gradient in place: hand it a buffer of its own)
                    dx, dW = torch.autograd.grad([y, alias], [x, W], [g, ga.clone()])
                else:
                    dx, dW = torch.autograd.grad([y], [x, W], [g])
                res += [y, dx, dW]
                wants.append((c, use_alias, ref.linear_passthrough(inp[0], inp[1], inp[2], inp[3] if use_alias else None)))
        res = fetch(res)
    for i, (c, use_alias, r) in enumerate(wants):
        for name, got in zip(("y", "dx", "dW"), res[3 * i:3 * i + 3]):
            assert ref.exact(got, r[name]), (c, use_alias, name)
