"""float64 NumPy restatement of the tail of a training step, own text: the KPFCNN cross entropy of csrc/loss.hip
(xent_*, ops.cross_entropy_lut) and the clip + momentum SGD of csrc/optim.hip (optim.FusedClipSGD), with the case tables
that tests/test_tail_cpu.py validates and tests/test_tail_gpu.py runs. NumPy only: no torch, no GPU.

Loss. A raw label l is renumbered through the int32 table `lut`: t = lut[clamp(l, -1, len(lut) - 2) + 1], so lut[0]
serves every negative label and lut[-1] every label above the table; the point is KEPT when 0 <= t < C. Over the kept
points, with w = 1 without class weights and g the upstream gradient:
    loss = sum_i w[t_i] (logsumexp(x_i) - x_i[t_i]) / sum_i w[t_i]           (0 / 0 = NaN when nothing is kept)
    dx_i = g w[t_i] / sum_j w[t_j] (softmax(x_i) - onehot(t_i)),             0 for a point that is not kept
Optimiser (torch.optim.SGD with dampening 0, no Nesterov, after clip_grad_value_):
    g' = clamp(g, -clip, clip) (a NaN stays a NaN; clip None: no clamp);  d = g' + wd p;  m = momentum m + d;  p = p - lr m
A parameter without a gradient is left alone, momentum included."""
import functools
import zlib

import numpy as np

XC_MAX = 256                 # csrc/loss.hip: the largest C it accepts
SGD_CHUNK = 4096             # csrc/optim.hip: elements per workgroup
EPS32 = 2.0 ** -24           # one float32 rounding, relative


def F(v):
    """The float32 nearest to v, as a Python float: hyper-parameters are float32 on the device, the oracle takes the same."""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------- the loss

def classes_of(labels, lut, C):
    """Class of every point, -1 for an ignored one (a table value < 0 or >= C counts as ignored)."""
    lut = np.asarray(lut).astype(np.int64)
    l = np.clip(np.asarray(labels).astype(np.int64), -1, lut.shape[0] - 2)
    t = lut[l + 1]
    return np.where((t >= 0) & (t < C), t, -1)


def xent64(logits, labels, lut, weight, g):
    """(loss, dlogits, kept_mask) in float64; loss is NaN (and dlogits all zero) when no point is kept."""
    x = np.asarray(logits, np.float64)
    N, C = x.shape
    t = classes_of(labels, lut, C)
    kept = t >= 0
    if not kept.any():
        return np.float64(np.nan), np.zeros_like(x), kept
    tt = np.where(kept, t, 0)
    w = np.ones(C, np.float64) if weight is None else np.asarray(weight, np.float64)
    w_t = np.where(kept, w[tt], 0.0)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = x.max(axis=1, keepdims=True)
        e = np.exp(x - m)
        s = e.sum(axis=1)
        lse = m[:, 0] + np.log(s)
        x_t = x[np.arange(N), tt]
        loss = np.float64(np.where(kept, w_t * (lse - x_t), 0.0).sum()) / np.float64(w_t.sum())
        onehot = (np.arange(C)[None, :] == tt[:, None]).astype(np.float64)
        k = np.float64(g) * w_t / np.float64(w_t.sum())
        dx = k[:, None] * (e / s[:, None] - onehot)
    return loss, np.where(kept[:, None], dx, 0.0), kept


def row_scale(labels, lut, weight, g, C):
    """g w[t_i] / sum_j w[t_j] of every point (0 for an ignored one): what a row of the gradient is a multiple of."""
    t = classes_of(labels, lut, C)
    kept = t >= 0
    w = np.ones(C, np.float64) if weight is None else np.asarray(weight, np.float64)
    w_t = np.where(kept, w[np.where(kept, t, 0)], 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.float64(g) * w_t / np.float64(w_t.sum())


def worst_row(dx, dx64, scale):
    """max over the rows with a finite non-zero scale of max_c |dx - dx64| / |scale|; 0.0 when there is no such row."""
    ok = np.isfinite(scale) & (scale != 0)
    if not ok.any():
        return 0.0
    d = np.abs(np.asarray(dx, np.float64)[ok] - np.asarray(dx64, np.float64)[ok]).max(axis=1)
    return float((d / np.abs(scale[ok])).max())


# logit scales: "r3" randn * 3; "shift" randn * 40 + 90 (exp overflows float32 without the max subtraction); "big"
# randn * 1e4; "ninf" randn * 3 with one class per row at -inf (never the row's own class); "const" every row constant
# lut kinds: "perm" C valid raw labels among 0 .. C + 5, both ends ignored; "ends" the same with lut[0] = class 0 and
# lut[-1] = class C - 1 (negative labels and labels above the table are KEPT); "edge" two more raw labels whose entries
# are C and C + 1 (ignored); "len3" the shortest table [-1, 0, C - 1]
# weights: "none"; "rand" in [0.5, 1.5); "zero1" rand with one present class at 0; "zeroall" every kept point in a class
# of weight 0 (0 / 0)
def _x(name, N, C, scale="r3", i64=True, lut="perm", weights="rand", g=1.7):
    return {"name": name, "N": N, "C": C, "scale": scale, "i64": i64, "lut": lut, "weights": weights, "g": g}


XENT_CASES = (
    # N across the seams: one wave (64), one workgroup (256), 64 workgroups = one partial per finishing lane (16384)
    [_x("n%d-c20" % n, n, 20, i64=bool(i % 2), weights=("rand", "none")[i % 3 == 2])
     for i, n in enumerate((1, 63, 64, 65, 255, 256, 257, 16384, 16385, 16641))]
    # C up to the limit
    + [_x("n257-c%d" % c, 257, c, i64=bool(i % 2), weights=("none", "rand")[i % 2]) for i, c in enumerate((1, 2, 13, 64, 255, 256))]
    + [_x("n16385-c256", 16385, 256, i64=False), _x("n65-c255", 65, 255, weights="none"), _x("n1-c1", 1, 1, weights="none"),
       _x("n16641-c1", 16641, 1, i64=False)]
    # logit scales
    + [_x("n%d-c%d-%s" % (n, c, s), n, c, scale=s, i64=i64)
       for s in ("shift", "big", "ninf", "const") for n, c, i64 in ((257, 20, True), (16641, 13, False))]
    + [_x("n255-c256-big", 255, 256, scale="big", weights="none"), _x("n64-c2-ninf", 64, 2, scale="ninf", i64=False),
       _x("n256-c256-shift", 256, 256, scale="shift", i64=False), _x("n63-c64-const", 63, 64, scale="const", weights="none")]
    # the table: entries >= C, its two ends live, the shortest table
    + [_x("n257-c13-edge", 257, 13, lut="edge", i64=False), _x("n16385-c20-edge", 16385, 20, lut="edge"),
       _x("n255-c13-ends", 255, 13, lut="ends", i64=False), _x("n256-c13-ends", 256, 13, lut="ends"),
       _x("n63-c1-len3", 63, 1, lut="len3"), _x("n256-c2-len3", 256, 2, lut="len3", i64=False)]
    # weights with zeros
    + [_x("n257-c13-zero1", 257, 13, weights="zero1"), _x("n16384-c20-zero1", 16384, 20, weights="zero1", i64=False),
       _x("n65-c13-zeroall", 65, 13, weights="zeroall", i64=False), _x("n16641-c2-zeroall", 16641, 2, weights="zeroall")]
    # upstream gradient
    + [_x("n256-c20-g1", 256, 20, g=1.0), _x("n256-c20-g0", 256, 20, g=0.0, i64=False),
       _x("n63-c64-g1", 63, 64, g=1.0, i64=False, weights="none"), _x("n16385-c13-g0", 16385, 13, g=0.0, weights="zero1")]
)
XENT_BY_NAME = {c["name"]: c for c in XENT_CASES}
assert len(XENT_BY_NAME) == len(XENT_CASES) <= 60


def _seed(name):
    return zlib.crc32(name.encode())


@functools.lru_cache(maxsize=None)
def xent_inputs(name):
    """The inputs of a case, drawn in float32 from a seed made of its name (read-only arrays): logits [N, C], labels [N]
    (int32 / int64 raw values), lut (int32), weight ([C] float32 or None), g, and `valid`, the raw label of every class."""
    c = XENT_BY_NAME[name]
    N, C = c["N"], c["C"]
    rng = np.random.default_rng(_seed(name))
    n = rng.standard_normal((N, C)).astype(np.float32)
    # the table
    if c["lut"] == "len3":
        assert C <= 2
        valid = np.arange(C, dtype=np.int64)                           # label 0 -> class 0, labels >= 1 -> class C - 1
        table = np.array([-1, 0, C - 1], np.int64)
        top = 0
    else:
        raw = np.sort(rng.choice(np.arange(0, C + 6), C + (2 if c["lut"] == "edge" else 0), replace=False))
        extra = rng.choice(raw.shape[0], 2, replace=False) if c["lut"] == "edge" else np.zeros(0, np.int64)
        valid = np.delete(raw, extra)
        top = int(raw.max())
        table = np.full(top + 3, -1, np.int64)
        table[valid + 1] = np.arange(C)
        for j, e in enumerate(extra):
            table[int(raw[e]) + 1] = C + j                           # C and C + 1: not classes
        if c["lut"] == "ends":
            table[0], table[-1] = 0, C - 1
    # the labels: three in four a class's raw label, the others anywhere in [-2, top + 4); every class once when
    # N >= 4 C; the out-of-table values at the front
    labels = valid[rng.integers(0, C, N)]
    other = rng.random(N) < 0.25
    labels[other] = rng.integers(-2, top + 4, int(other.sum()))
    if N >= 4 * C:
        labels[N - C:] = valid
    if N >= 8:
        labels[:4] = (-5, -1, top + 1, 2 ** 40 if c["i64"] else 2 ** 31 - 1)
    else:
        labels[0] = valid[-1]                                        # a single point: kept
    # the weights
    weight = None if c["weights"] == "none" else (rng.random(C) + 0.5).astype(np.float32)
    t = classes_of(labels, table, C)
    if c["weights"] == "zero1":
        weight[np.bincount(t[t >= 0], minlength=C).argmax()] = 0.0       # the most frequent class
    if c["weights"] == "zeroall":
        z = int(np.bincount(t[t >= 0], minlength=C).argmax())
        weight[z] = 0.0
        labels[(t >= 0) & (t != z)] = valid[z]                       # the kept points of the other classes: moved into it
        t = classes_of(labels, table, C)
    # the logits
    if c["scale"] == "r3":
        x = n * np.float32(3)
    elif c["scale"] == "shift":
        x = n * np.float32(40) + np.float32(90)
    elif c["scale"] == "big":
        x = n * np.float32(1e4)
    elif c["scale"] == "const":
        x = np.repeat(n[:, :1] * np.float32(3), C, axis=1)
    else:
        assert c["scale"] == "ninf" and C >= 2
        x = n * np.float32(3)
        x[np.arange(N), (np.where(t >= 0, t, 0) + 1 + np.arange(N) % (C - 1)) % C] = -np.inf
    out = {"logits": np.ascontiguousarray(x, np.float32), "labels": labels.astype(np.int64 if c["i64"] else np.int32),
           "lut": table.astype(np.int32), "weight": weight, "g": F(c["g"]), "valid": valid}
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def xent_expected(name):
    """xent64 of a case's inputs, computed once (read-only)."""
    i = xent_inputs(name)
    loss, dx, kept = xent64(i["logits"], i["labels"], i["lut"], i["weight"], i["g"])
    dx.setflags(write=False)
    kept.setflags(write=False)
    return loss, dx, kept


# ------------------------------------------------------------------------------------------------------ the optimiser

def clamp64(g, clip):
    """clamp(g, -clip, clip) that keeps a NaN; clip None: g itself."""
    g = np.asarray(g, np.float64)
    if clip is None:
        return g
    return np.where(g < -clip, -clip, np.where(g > clip, clip, g))


def clip_sgd64(p, g, m, lr, wd, momentum, clip):
    """One step on one tensor in float64: (p', m')."""
    p, m = np.asarray(p, np.float64), np.asarray(m, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = clamp64(g, clip) + wd * p
        m = momentum * m + d
        return p - lr * m, m


def effective_clip(clip_value):
    """The trainer's rule (utils/trainer.py:191): a bound that is None or <= 0 means no clipping."""
    return None if clip_value is None or clip_value <= 0 else float(clip_value)


SGD_LENGTHS = (1, 3, 4, 5, 4095, 4096, 4097, 8191, 8193, 15 * 66 * 64)
SGD_SHAPES = {n: (n,) for n in SGD_LENGTHS}
SGD_SHAPES[15 * 66 * 64] = (15, 66, 64)
BIG = 15 * 66 * 64
# The momentum views lie end to end in one flat buffer, so a view is 16-byte aligned when the lengths in front of it add
# up to a multiple of 4. "mis": the length-1 tensor first and the running sum never a multiple of 4 again -- every later
# tensor takes the scalar path. With lengths of every residue no single order aligns all ten tensors (a length of
# 3 mod 4 needs a start of 0 mod 4 and leaves 3 mod 4 behind); "al_a" and "al_b" swap the tensors of each pair, so that
# every tensor of 4 elements or more takes the float4 path in one of the two.
SGD_ORDERS = {
    "mis": (1, 4, 4096, BIG, 5, 3, 4097, 4095, 8193, 8191),
    "al_a": (4, 4096, BIG, 5, 3, 4097, 4095, 8193, 8191, 1),
    "al_b": (4, 4096, BIG, 3, 5, 4095, 4097, 8191, 8193, 1),
}
SGD_STEPS = 6
SGD_GROUPS = ({"lr": F(1e-2), "weight_decay": F(1e-3)}, {"lr": F(1e-3), "weight_decay": F(5e-4)})     # the first five tensors, the rest
SGD_NO_GRAD = (2, 8193)      # (step, length): the tensor that gets no gradient on that step


def _s(order, momentum, clip, offset_grad=()):
    name = "%s-m%g-clip%s%s" % (order, momentum, clip, "-off" if offset_grad else "")
    return {"name": name, "order": order, "momentum": F(momentum), "clip_value": clip, "offset_grad": tuple(offset_grad)}


# offset_grad: lengths whose float32 gradient is a view one element into its storage (4 bytes off: the scalar path)
SGD_CASES = (
    [_s("mis", m, 0.5) for m in (0.0, 0.9, 0.98)] + [_s("mis", 0.9, c) for c in (None, 0.0, -1.0)]
    + [_s("al_a", 0.9, 0.5), _s("al_a", 0.98, None), _s("al_a", 0.0, 0.5, offset_grad=(4096, 4097))]
    + [_s("al_b", 0.9, 0.5, offset_grad=(BIG, 4)), _s("al_b", 0.98, 0.0), _s("al_b", 0.0, -1.0)]
)
SGD_BY_NAME = {c["name"]: c for c in SGD_CASES}
assert len(SGD_BY_NAME) == len(SGD_CASES)


def sgd_vec_lengths(case):
    """The lengths whose tensor takes the float4 path in a case (parameter and gradient allocations are aligned):
    momentum view at a multiple of 4 elements, no offset gradient. A tensor shorter than 4 has no float4 to take."""
    out, off = set(), 0
    for n in SGD_ORDERS[case["order"]]:
        if off % 4 == 0 and n not in case["offset_grad"] and n >= 4:
            out.add(n)
        off += n
    return out


def sgd_group_of(k):
    return SGD_GROUPS[0 if k < 5 else 1]


@functools.lru_cache(maxsize=None)
def sgd_inputs(order):
    """(params, grads) of an order: params[k] float32 of SGD_SHAPES, grads[step][k] float32 or None. One seeded stream per
    order; the gradients alternate in scale (0.3 on even steps, 1.0 on odd ones)."""
    rng = np.random.default_rng(_seed("sgd-" + order))
    lens = SGD_ORDERS[order]
    params = [rng.standard_normal(SGD_SHAPES[n]).astype(np.float32) for n in lens]
    grads = []
    for step in range(SGD_STEPS):
        scale = np.float32(0.3 if step % 2 == 0 else 1.0)
        row = [(rng.standard_normal(SGD_SHAPES[n]).astype(np.float32) * scale) for n in lens]
        grads.append([None if (step, n) == SGD_NO_GRAD else g for n, g in zip(lens, row)])
    for a in params + [g for row in grads for g in row if g is not None]:
        a.setflags(write=False)
    return params, grads


def sgd_trajectory64(params, grads, momentum, clip_value, group_of=sgd_group_of):
    """[(p list, m list) after every step] in float64 from float32 inputs; clip_value by the trainer's rule."""
    clip = effective_clip(clip_value)
    p = [np.asarray(a, np.float64) for a in params]
    m = [np.zeros_like(a) for a in p]
    out = []
    for row in grads:
        for k, g in enumerate(row):
            if g is not None:
                grp = group_of(k)
                p[k], m[k] = clip_sgd64(p[k], g, m[k], grp["lr"], grp["weight_decay"], momentum, clip)
        out.append((list(p), list(m)))
    return out


@functools.lru_cache(maxsize=None)
def sgd_expected(name):
    c = SGD_BY_NAME[name]
    params, grads = sgd_inputs(c["order"])
    return sgd_trajectory64(params, grads, c["momentum"], c["clip_value"])


# ------------------------------------------------------------------------------------------------------ the joint head

HEAD = {"rows": 300, "features": 16, "classes": 7, "steps": 5, "slope": F(0.1), "g": F(1.7), "lr": F(0.05),
        "weight_decay": F(1e-3), "momentum": F(0.9), "clip_value": F(0.02)}


@functools.lru_cache(maxsize=None)
def head_inputs():
    """W [7, 16], b [7], per step x [300, 16] and raw labels [300] (int64), the table, class weights: float32, seeded."""
    h = HEAD
    rng = np.random.default_rng(_seed("joint-head"))
    W = (rng.standard_normal((h["classes"], h["features"])) / np.sqrt(h["features"])).astype(np.float32)
    b = (0.1 * rng.standard_normal(h["classes"])).astype(np.float32)
    valid = np.array([0, 1, 3, 4, 6, 7, 9], np.int64)               # raw labels 2, 5, 8 and everything outside: ignored
    lut = np.full(int(valid.max()) + 3, -1, np.int32)
    lut[valid + 1] = np.arange(h["classes"])
    xs = [rng.standard_normal((h["rows"], h["features"])).astype(np.float32) for _ in range(h["steps"])]
    labels = [rng.integers(-1, 12, h["rows"]).astype(np.int64) for _ in range(h["steps"])]
    weight = (rng.random(h["classes"]) + 0.5).astype(np.float32)
    return {"W": W, "b": b, "lut": lut, "xs": xs, "labels": labels, "weight": weight}


def head_trajectory64():
    """The chain linear + bias + LeakyReLU -> cross entropy (times g) -> clip + SGD in float64, 5 steps.
    Returns (W, b, losses, smallest |pre-activation| met)."""
    h, i = HEAD, head_inputs()
    W, b = i["W"].astype(np.float64), i["b"].astype(np.float64)
    mW, mb = np.zeros_like(W), np.zeros_like(b)
    losses, margin = [], np.inf
    for x, lab in zip(i["xs"], i["labels"]):
        x = x.astype(np.float64)
        v = x @ W.T + b
        margin = min(margin, float(np.abs(v).min()))
        y = np.where(v > 0, v, v * h["slope"])
        loss, dy, _ = xent64(y, lab, i["lut"], i["weight"], h["g"])
        d = dy * np.where(v > 0, 1.0, h["slope"])
        W, mW = clip_sgd64(W, d.T @ x, mW, h["lr"], h["weight_decay"], h["momentum"], h["clip_value"])
        b, mb = clip_sgd64(b, d.sum(0), mb, h["lr"], h["weight_decay"], h["momentum"], h["clip_value"])
        losses.append(float(loss))
    return W, b, losses, margin
