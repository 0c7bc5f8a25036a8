"""Oracle of the GEMM family of csrc/gemm.hip: NumPy restatements in int64 / float64 of every product the library
fuses, a Python restatement of the host's choice of loader path, and the case lists as data. NumPy only; nothing here
touches a device, and no expected value anywhere comes from a launch of the kernel under test.

TWO INPUT FAMILIES

  I (exact)     every operand, bias, upstream gradient and accumulate base holds integers in [-4, 4] stored as float32,
                LeakyReLU slopes are 1.0 or 0.25. Every product and every partial sum, in any order, is then an integer
                (or a multiple of 1/4) far below 2^24: float32 arithmetic is exact, so the MFMA chain, the f32 atomics of
                a split, the ordered split, the scatter epilogue and the column sums of the statistics epilogue must
                give the NumPy result BIT FOR BIT (`exact`). The precondition -- max over the outputs of sum |a||b|, times
                the number of splits where a base is added, plus the base, below 2^24 -- is `precondition`; the CPU test
                asserts it for every case.
  R (rounding)  float32 normals, the rows of op(A) and the columns of op(B) scaled by 10^U(-3, 3) (small and large outputs
                in one matrix), column 0 of op(A) a constant 40 before the scaling (column means far from zero). The rule is
                per element: |got - f64| <= (K_total + 4) 2^-24 (|A|.|B|)_ij (`r_bound`): the worst case of a dot product
                of K_total terms summed in any order with fused or unfused multiply-adds in round-to-nearest -- derived,
                not measured, no margin. Family R is used for plain products only (no bias, no base: their magnitudes are
                not part of the bound as stated).

THE HOST'S PATH CHOICE (`path`) restates vec_width, Tile::fast_ok, the pipeline selection of gemm_body, plan_gemm's tile
class under MVK_GEMM_FORCE and clamp_split. The GPU test does not trust it for correctness; the case lists use it to
PROVE which loader paths they reach (tests/test_gemm_ref_cpu.py).

One property of the host logic shapes the lists: ops.gemm hands the split it was given on to mvk_gemm_f32_ex as an
explicit request, and plan_gemm honours an explicit request only while every workgroup keeps >= 4 k-tiles
(ksteps // split >= 4); otherwise the product runs unsplit. A plain product therefore never has fewer than four full
k-tiles per split when it is split at all, and a requested split larger than the k-tile count reaches clamp_split only
through the entry points that plan for themselves (gemm_ldb, gemm_dual, ...), where MVK_GEMM_FORCE sets the split
unconditionally: LDB_CASES and DUAL_CASES carry those.

OUT OF SCOPE (tests/test_gemm_oracle_gpu.py repeats the reasons): the operand transform and finished statistics
(mvk_gemm_f32_bn, mvk_gemm_f32_pair_bn: tests/test_bn_fold_gpu.py), the streaming kernel of csrc/gemm32s.hip (not planned
below 4 096 rows; it has its own float64 test), graph capture of the grouped launch (the existing test covers it).
"""
import collections
import zlib

import numpy as np

BK = 32
U = 2.0 ** -24                       # unit roundoff of float32
EXACT_LIMIT = 2 ** 24
LAYOUTS = ("NN", "NT", "TN", "TT")
WIDE_FORCES = ((1, 1), (2, 1), (4, 1), (5, 1), (1, 2), (2, 2), (4, 2))
NARROW_FORCES = ((1, 0), (2, 0))     # pm; qn of the narrow class follows from N (<= 16: 1, else 2)


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------ host path choice

def vec_width(off, ld):
    """Floats per load of an operand that starts `off` floats past a 16-byte boundary with rows `ld` floats apart."""
    return 4 if (ld % 4 == 0 and off % 4 == 0) else 2 if (ld % 2 == 0 and off % 2 == 0) else 1


def fast_ok(contig_k, imax, vec):
    return (vec >= 2 and imax >= 1) if contig_k else (vec == 4 and imax >= 4 and imax % 4 == 0)


def clamp_split(Kd, split):
    """(number of splits, k per split) a reduction of Kd gets when `split` is asked for."""
    ksteps = cdiv(Kd, BK)
    split = min(split, ksteps)
    kps = cdiv(ksteps, split) * BK
    return cdiv(Kd, kps), kps


def honoured_split(Kd, split):
    """The split of a plain ops.gemm product asked for `split` (see the module docstring)."""
    return split if split <= 1 or cdiv(Kd, BK) // split >= 4 else 1


def tile_class(N, force=None, want_stats=False):
    """(narrow, pm, qn, tm, tn) of plan_gemm under MVK_GEMM_FORCE = force (pm, qn, split; 0 = the plan's own)."""
    narrow = N <= 32
    pm = 1 if narrow else (4 if want_stats else 2)
    qn = (1 if N <= 16 else 2) if narrow else 1
    if force:
        if force[0] > 0:
            pm = force[0]
        if force[1] > 0 and not narrow:
            qn = force[1]
    return narrow, pm, qn, (64 * pm if narrow else 16 * pm), (16 * qn if narrow else 64 * qn)


Path = collections.namedtuple("Path", "vecA vecB fastA fastB pipeline nsplit k_per_split parts narrow pm qn tm tn")


def path(layout, M, N, K, offA=0, offB=0, force=None, explicit_request=True):
    """The loader path of op(A) [M,K] . op(B) [K,N]: parts = ((full k-tiles, has tail), ...) per split. explicit_request:
    the split of `force` arrives as ops.gemm's request (honoured_split); False: the entry point plans for itself."""
    ta, tb = layout[0] == "T", layout[1] == "T"
    lda, ldb = (M if ta else K), (K if tb else N)
    vA, vB = vec_width(offA, lda), vec_width(offB, ldb)
    fA, fB = fast_ok(not ta, M, vA), fast_ok(tb, N, vB)
    pipe = "44" if (fA and fB and vA == 4 and vB == 4) else "24" if (fA and fB and vA == 2 and vB == 4) else "general"
    want = force[2] if force and force[2] > 0 else 1
    if K == 0:                                   # no launch: the host zero-fills
        return Path(vA, vB, fA, fB, pipe, 1, 0, (), *tile_class(N, force))
    n, kps = clamp_split(K, honoured_split(K, want) if explicit_request else want)
    parts = []
    for z in range(n):
        k0, k1 = z * kps, min((z + 1) * kps, K)
        parts.append(((k1 - k0) // BK, (k1 - k0) % BK != 0))
    return Path(vA, vB, fA, fB, pipe, n, kps, tuple(parts), *tile_class(N, force))


def launchable(N, force):
    """Whether launch_cfg has an instantiation for the forced tile."""
    narrow, pm, qn = tile_class(N, force)[:3]
    return (pm, qn) in (((1, 1), (2, 1), (1, 2), (2, 2)) if narrow else WIDE_FORCES)


# ------------------------------------------------------------------------------------------ restatements

def wide(x):
    """int64 where the values are integers (Family I), float64 otherwise."""
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        return x.astype(np.int64)
    return x.astype(np.int64) if np.array_equal(x, np.rint(x)) else x.astype(np.float64)


def op(X, t):
    return X.T if t else X


def product(A, B, layout="NN", base=None):
    """op(A) . op(B) (+ base: `accumulate`)."""
    C = op(wide(A), layout[0] == "T") @ op(wide(B), layout[1] == "T")
    return C if base is None else C + wide(base)


def abs_product(A, B, layout="NN"):
    return op(np.abs(np.asarray(A, np.float64)), layout[0] == "T") @ op(np.abs(np.asarray(B, np.float64)), layout[1] == "T")


def lrelu(v, slope):
    v = np.asarray(v, np.float64)
    return np.where(v > 0, v, v * slope)


def linear_bias_lrelu(x, W, b, slope, g):
    """y = LeakyReLU(x W^T + b) and the gradients of x, W, b under the upstream gradient g; also the pre-activation."""
    v = (wide(x) @ wide(W).T + wide(b)).astype(np.float64)
    d = np.asarray(g, np.float64) * np.where(v > 0, 1.0, slope)
    return {"pre": v, "y": lrelu(v, slope), "dx": d @ np.asarray(W, np.float64), "dW": d.T @ np.asarray(x, np.float64),
            "db": d.sum(0)}


def linear_pair(x, W0, W1, g0, g1):
    x, W0, W1, g0, g1 = (wide(t) for t in (x, W0, W1, g0, g1))
    return {"y0": x @ W0.T, "y1": x @ W1.T, "dx": g0 @ W0 + g1 @ W1, "dW0": g0.T @ x, "dW1": g1.T @ x}


def gemm_dual(A, B, A2, B2):
    return wide(A) @ wide(B) + wide(A2) @ wide(B2)


def upsample_cat_linear(x, idx, skip, W, g):
    """y = cat([xpad[idx[:, 0]], skip], 1) W^T with xpad = x and one zero row (entries outside [0, Ns) are shadows) and
    the gradients of x (a scatter-add over idx[:, 0]), skip and W."""
    x, skip, W, g = (wide(t) for t in (x, skip, W, g))
    Ns, C1 = x.shape
    j = np.asarray(idx).reshape(len(idx), -1)[:, 0].astype(np.int64)
    j = np.where((j < 0) | (j >= Ns), Ns, j)
    cat = np.concatenate([np.concatenate([x, np.zeros_like(x[:1])])[j], skip], 1)
    gc = g @ W
    dx = np.zeros((Ns + 1, C1), gc.dtype)
    np.add.at(dx, j, gc[:, :C1])
    return {"y": cat @ W.T, "dx": dx[:Ns], "dskip": gc[:, C1:], "dW": g.T @ cat}


def kp_transposed_contraction(A2, W):
    """dx [M, Cin] = sum_k A2[:, k, :] . W[k]^T for A2 [M, K, Cout], W [K, Cin, Cout]."""
    return np.einsum("mko,kco->mc", wide(A2), wide(W))


def gemm_ldb(A, Bwide, col0, N):
    return wide(A) @ wide(Bwide)[:, col0:col0 + N]


def linear_passthrough(x, W, g, g_alias=None):
    """y = x W^T beside an alias of x for a second consumer: dx = g W (+ the alias' gradient), dW = g^T x."""
    x, W, g = wide(x), wide(W), wide(g)
    dx = g @ W
    return {"y": x @ W.T, "dx": dx if g_alias is None else dx + wide(g_alias), "dW": g.T @ x}


def stats_partials(C, n_valid, rows):
    """The statistics epilogue in float64: per block of `rows` rows of C the column sum and the sum of squares about the
    block's own mean over the rows below n_valid -> (sums [blocks, N], m2 [blocks, N], counts [blocks])."""
    C = np.asarray(C, np.float64)
    M, N = C.shape
    nb = cdiv(M, rows)
    sums, m2, cnt = np.zeros((nb, N)), np.zeros((nb, N)), np.zeros(nb, np.int64)
    for b in range(nb):
        blk = C[b * rows:min((b + 1) * rows, M, max(n_valid, 0))] if b * rows < n_valid else C[:0]
        cnt[b] = blk.shape[0]
        if blk.shape[0]:
            sums[b] = blk.sum(0)
            m2[b] = ((blk - blk.mean(0)) ** 2).sum(0)
    return sums, m2, cnt


def m2_bound(m2, sums, cnt, rows):
    """|m2_got - m2| allowed: (rows per block + 8) 2^-24 relative plus n (2^-24 |mean|)^2 absolute -- the kernel sums the
    squares about the block mean ROUNDED to float32 (an offset d of the centre adds n d^2), in float32."""
    n = np.asarray(cnt, np.float64)[:, None]
    mean = np.where(n > 0, sums / np.maximum(n, 1), 0.0)
    return (rows + 8) * U * m2 + n * (U * np.abs(mean)) ** 2


# ------------------------------------------------------------------------------------------ comparison rules

def exact(got, want):
    """Family I: every element equal (the reference holds integers or multiples of 1/4: exact in float32)."""
    got, want = np.asarray(got), np.asarray(want)
    return got.shape == want.shape and bool(np.isfinite(got.astype(np.float64)).all()) \
        and np.array_equal(got.astype(np.float64), want.astype(np.float64))


def precondition(absprod, nsplit=1, base=None):
    """Family I: the largest magnitude any partial sum can reach (a base is added once per split at worst)."""
    top = float(np.max(absprod)) if np.size(absprod) else 0.0
    if base is not None:
        top = top * nsplit + float(np.max(np.abs(base)))
    return top


def r_bound(absprod, k_total):
    return (k_total + 4) * U * np.asarray(absprod, np.float64)


def r_ratio(got, want, absprod, k_total):
    """Family R: the largest |got - want| / bound over the elements (<= 1 passes; inf for a non-finite element)."""
    got = np.asarray(got, np.float64)
    if got.shape != np.shape(want) or not np.isfinite(got).all():
        return np.inf
    if got.size == 0:
        return 0.0
    b = r_bound(absprod, k_total)
    err = np.abs(got - np.asarray(want, np.float64))
    return float(np.max(np.where(b > 0, err / np.where(b > 0, b, 1.0), np.where(err > 0, np.inf, 0.0))))


# ------------------------------------------------------------------------------------------ inputs

def rng_of(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def ints(rng, *shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def r_operands(rng, M, N, K):
    """op(A) [M,K], op(B) [K,N] of Family R."""
    A = rng.standard_normal((M, K)).astype(np.float32)
    A[:, 0] = 40.0
    A = (A * (10.0 ** rng.uniform(-3, 3, (M, 1))).astype(np.float32)).astype(np.float32)
    B = (rng.standard_normal((K, N)).astype(np.float32) * (10.0 ** rng.uniform(-3, 3, (1, N))).astype(np.float32)).astype(np.float32)
    return A, B


Case = collections.namedtuple("Case", "layout M N K offA offB force family accumulate")


def case_id(c):
    return "%s-%dx%dx%d-a%db%d-f%d.%d.%d-%s%s" % (c.layout, c.M, c.N, c.K, c.offA, c.offB, *c.force, c.family,
                                                  "-acc" if c.accumulate else "")


def operands(c):
    """A, B as stored (A [K,M] when transposed, B [N,K] when transposed) and the accumulate base or None."""
    rng = rng_of(*c)
    if c.family == "I":
        A, B = ints(rng, c.M, c.K), ints(rng, c.K, c.N)
    else:
        A, B = r_operands(rng, c.M, c.N, c.K)
    base = ints(rng, c.M, c.N) if c.accumulate else None
    return (np.ascontiguousarray(op(A, c.layout[0] == "T")), np.ascontiguousarray(op(B, c.layout[1] == "T")), base)


# ------------------------------------------------------------------------------------------ the plain-product list

FULL_TILES = (0, 1, 2, 3, 5)


def reachable_pipelines(layout):
    """(2,4) needs a k-contiguous A (the row-contiguous fast loader is float4 only) and a B at vec 4: NN, and NT when A
    starts 8 bytes off a 16-byte boundary (lda = ldb = K there, so only the base offset can tell the operands apart)."""
    return ("44", "24", "general") if layout in ("NN", "NT") else ("44", "general")


def _pipeline_case(layout, pipe, t, tail, n):
    """One unsplit Family-I case of `layout` on `pipe` with t full k-tiles and (or not) a ragged tail."""
    ta, tb = layout[0] == "T", layout[1] == "T"
    k_is_ld = (not ta) or tb                      # K is the row stride of an operand
    offA = offB = 0
    M, N = (36 if ta else 33), (70 if tb else 68)
    if pipe == "44":
        K = BK * t + ((12 if k_is_ld else 13) if tail else 0)
    elif pipe == "24":
        if layout == "NT" or not tail or t % 2:
            K, offA = BK * t + (8 if tail else 0), 2          # via the base offset
        else:
            K = BK * t + 6                                     # via the stride: K % 4 == 2
    else:
        K = BK * t + ((12 if k_is_ld else 13) if tail else 0)
        why = t % 3
        if why == 0:
            offA = 1
        elif why == 1:
            offB = 1
        elif layout == "NT":
            offA = offB = 2                                    # both at vec 2: no fast pair
        elif layout == "NN":
            N = 70                                             # B at vec 2
        else:
            M = 34 if layout == "TT" else 33                   # a transposed A off float4 rows
    force = ((WIDE_FORCES[n % len(WIDE_FORCES)]) + (1,))
    c = Case(layout, M, N, K, offA, offB, force, "I", False)
    p = path(*c[:6], force=force)
    assert p.pipeline == pipe and p.parts == ((t, tail),), (c, p)
    return c


def _plain_cases():
    out = []
    # (1) every reachable pipeline x full k-tiles x tail, per layout; K = 0 (0 full, no tail) never launches
    for layout in LAYOUTS:
        for pipe in reachable_pipelines(layout):
            for t in FULL_TILES:
                for tail in (False, True):
                    if t or tail:
                        out.append(_pipeline_case(layout, pipe, t, tail, len(out)))
        out.append(Case(layout, 5, 40, 0, 0, 0, (2, 1, 1), "I", False))
    # (2) every forced plan x splits 1 / 2 / 3 per layout: 13 k-tiles and a tail -> split 3 is 5 + 5 + (3 + tail): ragged
    for layout in LAYOUTS:
        for pm, qn in WIDE_FORCES + NARROW_FORCES:
            for split in (1, 2, 3):
                wide_ = qn > 0
                tm = 16 * pm if wide_ else 64 * pm
                M = tm + (4 if layout[0] == "T" else 5)
                Ns = ((64 * qn + 4,) if wide_ else (12, 20))
                for N in Ns:
                    K = 13 * BK + (12 if (len(out) % 2) else 0)
                    off = (0, 0) if len(out) % 3 else (len(out) % 2 + 1, 0)
                    out.append(Case(layout, M, N, K, off[0], off[1], (pm, qn, split), "I", (len(out) // 2) % 2 == 0))
    # (3) M and N at 1, tile - 1, tile, tile + 1 of every tile class (N decides the class: a narrow class ends at its
    # tile width, and N = 1 is always the 16-column narrow class), two full k-tiles and a tail of 8, rotating layouts
    for pm, qn in WIDE_FORCES + NARROW_FORCES:
        for N0 in ((64 * qn,) if qn else (16, 32)):
            cls = tile_class(N0, (pm, qn, 1))
            tm, tn = cls[3:]
            assert tn == N0
            pairs = [(m, tn) for m in (1, tm - 1, tm, tm + 1)] + [(tm + 1, n) for n in (1, tn - 1, tn + 1)]
            for m, n in pairs:
                if tile_class(n, (pm, qn, 1)) != cls:
                    continue                       # these columns belong to another class (UNREACHABLE_EDGES)
                out.append(Case(LAYOUTS[len(out) % 4], m, n, 72, 0, 0, (pm, qn, 1), "I", False))
    # (4) every operand at vec 4 / 2 / 1 by its stride and by its base offset (NN: lda = K, ldb = N; TT: lda = M, ldb = K)
    for K, N, oa, ob in ((72, 68, 0, 0), (70, 68, 0, 0), (71, 68, 0, 0), (72, 68, 2, 0), (72, 68, 1, 0), (72, 70, 0, 0),
                         (72, 71, 0, 0), (72, 68, 0, 2), (72, 68, 0, 1), (72, 68, 3, 3)):
        out.append(Case("NN", 33, N, K, oa, ob, (2, 1, 1), "I", False))
    for M, K, oa, ob in ((36, 72, 0, 0), (34, 70, 0, 0), (33, 71, 0, 0), (36, 72, 2, 2), (36, 72, 1, 1)):
        out.append(Case("TT", M, 68, K, oa, ob, (2, 1, 1), "I", False))
    # (5) Family R: the rule per element, on every layout, both tile classes, unsplit and split, fast and general loaders
    for layout in LAYOUTS:
        for (M, N, K, oa, force) in ((36, 68, 13 * BK + 12, 0, (2, 1, 1)), (36, 68, 13 * BK + 12, 0, (2, 1, 3)),
                                     (33, 70, 203, 1, (4, 1, 1)), (68, 20, 13 * BK, 0, (1, 0, 2)), (7, 130, 5, 0, (1, 2, 1)),
                                     (100, 12, 990, 2, (2, 0, 3))):
            out.append(Case(layout, M, N, K, oa, 0, force, "R", False))
    assert len(set(out)) == len(out)
    return out


PLAIN_CASES = _plain_cases()

# ------------------------------------------------------------------------------------------ the fused forms' lists

BIAS_SHAPES = [(M, N, K) for M in (1, 5, 33, 70) for N in (7, 20, 33, 64) for K in (16, 33, 64)]
BIAS_SLOPES = (1.0, 0.25)

# (M, N0, N1, Kd, with stats): None expected for the Kd > 512 narrow partner
PAIR_CASES = [(1030, 32, 128, 64, True), (1030, 32, 128, 64, False), (70, 64, 128, 33, False), (70, 64, 128, 600, False),
              (1030, 48, 68, 40, True), (70, 48, 68, 40, False), (130, 50, 70, 33, True), (33, 32, 64, 512, False)]
PAIR_NONE = (70, 32, 128, 544)

DUAL_CASES = [(33, 64, 32, 1), (70, 68, 64, 33), (70, 128, 96, 100), (1, 33, 32, 31)]
DUAL_NONE = [(33, 64, 48, 32), (33, 20, 32, 32)]

# (Ns, Nq, C1, C2, Cout)
UPCAT_CASES = [(7, 70, 4, 4, 64), (30, 100, 30, 7, 16), (5, 33, 64, 33, 48), (40, 200, 36, 28, 128)]
UPCAT_INDEX_KINDS = ("random", "all_shadow", "one_row")

# (M, K, Cin, Cout)
KP_CASES = [(1, 1, 1, 32), (33, 3, 5, 32), (70, 15, 7, 64), (70, 2, 66, 128), (33, 3, 7, 45)]

# (M, Kd, col0, N, ldb, forced split or 0); the last two ask for more splits than there are k-tiles
LDB_CASES = [(33, 40, c0, N, c0 + N + extra, 0) for c0 in (0, 1, 2, 4) for N, extra in ((4, 1), (20, 4), (64, 2), (66, 3))] \
    + [(33, 40, 4, 64, 72, 3), (5, 33, 0, 20, 24, 7)]

# (M, N, K, forced split (ordered mode only) or 1): M just above ops.bn_single_launch_rows(N) = 1024 (N % 4 == 0) or 128
STATS_CASES = [(1030, 64, 40, 1), (200, 66, 40, 1), (1030, 20, 33, 1), (150, 18, 33, 1), (150, 7, 20, 1), (1090, 128, 16, 1),
               (1030, 64, 256, 2), (150, 18, 256, 2)]

# weight gradients dW [M,N] = A^T [M,Kd] . B [Kd,N]: (Kd, M, N)
DW_CASES = [(1, 1, 17), (31, 15, 32), (33, 64, 33), (200, 70, 64), (1100, 70, 130), (1100, 15, 17), (200, 1, 130),
            (33, 70, 32), (31, 64, 64), (1, 70, 33), (1100, 64, 32), (33, 15, 130)]
DW_SMALL = (200, 15, 9)               # N <= 16: not grouped, computed at once

# (M, N, K) of linear(..., passthrough=True)
PASS_CASES = [(33, 20, 16), (70, 64, 33), (5, 130, 64)]


# ------------------------------------------------------------------------------------------ Family-I inputs of the fused forms

def bias_inputs(M, N, K):
    """x [M,K], W [N,K], b [N], g [M,N]; output column 0 has pre-activation exactly 0 in every row, column 1 is negative."""
    rng = rng_of("bias", M, N, K)
    x, W, b, g = ints(rng, M, K), ints(rng, N, K), ints(rng, N), ints(rng, M, N)
    W[0], b[0] = 0, 0
    W[1], b[1] = 0, -3
    return x, W, b, g


def pair_inputs(M, N0, N1, Kd):
    rng = rng_of("pair", M, N0, N1, Kd)
    return ints(rng, M, Kd), ints(rng, N0, Kd), ints(rng, N1, Kd), ints(rng, M, N0), ints(rng, M, N1)


def dual_inputs(M, N, Kd, Kd2):
    rng = rng_of("dual", M, N, Kd, Kd2)
    return ints(rng, M, Kd), ints(rng, Kd, N), ints(rng, M, Kd2), ints(rng, Kd2, N)


def upcat_inputs(Ns, Nq, C1, C2, Cout, kind):
    """x [Ns,C1], idx [Nq,3] int64 (only column 0 counts; the others hold other valid entries), skip [Nq,C2],
    W [Cout,C1+C2], g [Nq,Cout]. Shadow entries are Ns."""
    rng = rng_of("upcat", Ns, Nq, C1, C2, Cout, kind)
    idx = rng.integers(0, Ns + 1, size=(Nq, 3)).astype(np.int64)
    if kind == "random":
        idx[:, 0] = np.minimum(rng.integers(0, Ns + Ns // 3 + 2, size=Nq), Ns)
        idx[0, 0], idx[Nq - 1, 0] = Ns, 0
    elif kind == "all_shadow":
        idx[:, 0] = Ns
    else:
        idx[:, 0] = Ns // 2
    return ints(rng, Ns, C1), idx, ints(rng, Nq, C2), ints(rng, Cout, C1 + C2), ints(rng, Nq, Cout)


def kp_inputs(M, K, Cin, Cout):
    rng = rng_of("kp", M, K, Cin, Cout)
    return ints(rng, M, K, Cout), ints(rng, K, Cin, Cout)


def ldb_inputs(M, Kd, ldb):
    rng = rng_of("ldb", M, Kd, ldb)
    return ints(rng, M, Kd), ints(rng, Kd, ldb)


def stats_inputs(M, N, K, family):
    """A [M,K], B [K,N]; family "N": plain normals with column 0 of A = 40 (the data of the existing statistics tests)."""
    rng = rng_of("stats", M, N, K, family)
    if family == "I":
        return ints(rng, M, K), ints(rng, K, N)
    A, B = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    A[:, 0] = 40.0
    return A, B


def dw_inputs(Kd, M, N):
    rng = rng_of("dw", Kd, M, N)
    return ints(rng, Kd, M), ints(rng, Kd, N)


def pass_inputs(M, N, K):
    rng = rng_of("pass", M, N, K)
    return ints(rng, M, K), ints(rng, N, K), ints(rng, M, N), ints(rng, M, K)


def top_magnitude(result):
    """Largest magnitude in a restatement's result (an array or a dict of arrays): called on the restatement of the
    ABSOLUTE inputs it is the largest partial sum any summation order can meet."""
    vals = result.values() if isinstance(result, dict) else [result]
    return max((float(np.max(np.abs(v))) for v in vals if np.size(v)), default=0.0)
