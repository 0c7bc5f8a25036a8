"""Float64 oracle of the masked BatchNorm + LeakyReLU (csrc/bn.hip), the per-channel referee comparator and the case
table, own text. NumPy float64 throughout; nothing here touches a device (`ref32` runs torch on the device it is given).

The operation (models/blocks.py:430-467, :644-649): over the first n rows of x [R, D]

    mean, var (biased), invstd = 1 / sqrt(var + eps),   xh = (x - mean) * invstd,   z = xh * gamma + beta (+ addend),
    y = z (z > 0) or slope * z,    g' = go * (1 or slope),    dbeta = sum g',    dgamma = sum g' xh,
    dx = gamma * invstd * (g' - dbeta / n - xh * dgamma / n),    d_addend = g',
    running_mean <- (1 - m) running_mean + m mean,    running_var <- (1 - m) running_var + m var n / (n - 1)

(n = 1: the running variance takes the biased value, 0, as the kernels do; nn.BatchNorm1d refuses one row). Rows >= n of
y, dx and d_addend are zero.

THE KINK IS DECIDED ONCE. With mag = |xh gamma| + |beta| + |addend|, the elements with |z| <= BAND * mag are "in the
band": a last-bit difference of the normalised value may put them on either side of the LeakyReLU. There the oracle
takes the side of the implementation it is judging (y_impl > 0); everywhere else its own z > 0. An implementation that
flips an element outside the band therefore shows up as a gradient error, and one inside cannot fail a column sum. The
share of in-band elements is returned and is capped at BAND_SHARE_MAX per case (a condition on the CASES, asserted in
tests/test_bn_ref_cpu.py; a case that breaks it gets another seed, not a wider cap).

DENOMINATORS COME FROM THE ORACLE, per channel, not from the compared tensor (for n = 2, dx cancels to rounding noise
and its own norm means nothing):

    y          || mag[:, c] ||                      dgamma[c]   sum |g' xh|           mean[c]   |mean| + sqrt(var)
    dx         || (gamma invstd g')[:, c] ||        dbeta[c]    sum |g'|              var[c]    var + eps
    d_addend   || g'[:, c] ||                       running statistics: the magnitudes of the two terms of the update

`compare` holds every channel of every tensor to the project's referee rule (tests/util.py, where the two constants
and their reasons live): err_c(impl, f64) <= REFEREE_FACTOR * err_c(ref32, f64) + REFEREE_FLOOR, err_c = the channel's
L2 difference over the scale (2-D tensors) or the absolute difference over the scale (per-channel vectors). ref32 is a
float32 run of the plain tensor expression on the device of the implementation. Each judged implementation gets its own
evaluation of the oracle, hence its own kink decisions.

OUT OF SCOPE:
  * bn_lrelu_pair: bit-equal to two single launches (test_bn_lrelu_pair_equals_two_single_launches);
  * statistics finished by the producer and the operand fold (ext_rows = -1, MVK_BN_FOLD): off by default, covered by
    tests/test_bn_fold_gpu.py;
  * synchronised BatchNorm (tensor ops, tests/test_model_gpu.py);
  * a row 0 that is an outlier of its column: the kernels shift by row 0 by design (csrc/bn.hip:8); row 0 is an
    ordinary sample in every case here, and nothing here probes or changes the shift.
"""
import collections

import numpy as np

from util import REFEREE_FACTOR, REFEREE_FLOOR, check_err

BAND = 1e-4                 # |z| <= BAND * mag: the LeakyReLU side is the judged implementation's
BAND_SHARE_MAX = 1e-3       # of the valid elements of a case
EPS = 1e-5                  # nn.BatchNorm1d's default
MOMENTUM = 0.02             # the network's (blocks.py: 1 - 0.98)
TINY = 1e-300

TENSORS_2D = ("y", "dx", "d_addend")
TENSORS_1D = ("dgamma", "dbeta", "mean", "var", "running_mean", "running_var")

Oracle = collections.namedtuple("Oracle", "n mean var invstd xh y dx d_addend dgamma dbeta running_mean running_var "
                                          "band_share scales")


def oracle(x, n, gamma, beta, eps, slope, addend, go, y_impl, running=None, momentum=None, updates=1):
    """The float64 values and per-channel scales described in the module docstring. x, go, addend (or None), y_impl
    [R, D] (y_impl: at least its first n rows); running = (running_mean, running_var) before the first of `updates`
    identical updates (None: not tracked). 2-D results have R rows, zero from row n on."""
    x, go = np.asarray(x, np.float64), np.asarray(go, np.float64)
    gamma, beta = np.asarray(gamma, np.float64), np.asarray(beta, np.float64)
    R, D = x.shape
    assert 1 <= n <= R and go.shape == x.shape and np.shape(y_impl)[0] >= n and np.shape(y_impl)[1] == D
    xv, gv = x[:n], go[:n]
    ad = np.zeros_like(xv) if addend is None else np.asarray(addend, np.float64)[:n]
    mean = xv.mean(0)
    var = ((xv - mean) ** 2).mean(0)
    invstd = 1.0 / np.sqrt(var + eps)
    xh = (xv - mean) * invstd
    z = xh * gamma + beta + ad
    mag = np.abs(xh * gamma) + np.abs(beta) + np.abs(ad)
    band = np.abs(z) <= BAND * mag
    positive = np.where(band, np.asarray(y_impl)[:n] > 0, z > 0)
    factor = np.where(positive, 1.0, float(slope))
    gp = gv * factor
    dbeta = gp.sum(0)
    dgamma = (gp * xh).sum(0)
    dx = gamma * invstd * (gp - dbeta / n - xh * dgamma / n)
    scales = {"y": np.linalg.norm(mag, axis=0), "dx": np.linalg.norm(gamma * invstd * gp, axis=0),
              "d_addend": np.linalg.norm(gp, axis=0), "dgamma": np.abs(gp * xh).sum(0), "dbeta": np.abs(gp).sum(0),
              "mean": np.abs(mean) + np.sqrt(var), "var": var + eps}
    rm = rv = None
    if running is not None:
        rm, rv = np.asarray(running[0], np.float64), np.asarray(running[1], np.float64)
        unbiased = var * (n / (n - 1.0)) if n > 1 else var
        for _ in range(updates):
            scales["running_mean"] = np.abs((1 - momentum) * rm) + np.abs(momentum * mean)
            scales["running_var"] = np.abs((1 - momentum) * rv) + np.abs(momentum * unbiased)
            rm = (1 - momentum) * rm + momentum * mean
            rv = (1 - momentum) * rv + momentum * unbiased

    def padded(a):
        out = np.zeros((R, D))
        out[:n] = a
        return out

    return Oracle(n, mean, var, invstd, padded(xh), padded(z * factor), padded(dx), padded(gp), dgamma, dbeta, rm, rv,
                  float(band.mean()), scales)


def channel_errors(name, got, o):
    """err_c of one tensor against the oracle o: [D] float64."""
    want, scale = getattr(o, name), np.maximum(o.scales[name], TINY)
    got = np.asarray(got, np.float64)
    if name in TENSORS_2D:
        return np.linalg.norm(got[:o.n] - want[:o.n], axis=0) / scale
    return np.abs(got - want) / scale


def compare(label, impl, ref32, oracle_of, failures=None):
    """The referee rule per channel for every tensor of `impl` (a dict name -> array; 2-D tensors with at least n rows).
    ref32: the same dict from the float32 reference, or None (n = 1: the referee term is zero). oracle_of(y) -> Oracle
    evaluates the oracle with the kink decisions of the implementation whose output is y. The worst channel of every
    tensor goes through util.check_err (measured value next to its bound in the parity log). failures: a dict that
    collects {tensor: failing channels} instead of raising. Returns {tensor: (err, bound) of the worst channel}."""
    o_impl = oracle_of(impl["y"])
    o_ref = oracle_of(ref32["y"]) if ref32 is not None else None
    report, lines = {}, []
    for name in TENSORS_2D + TENSORS_1D:
        if impl.get(name) is None:
            continue
        e_impl = channel_errors(name, impl[name], o_impl)
        e_ref = channel_errors(name, ref32[name], o_ref) if o_ref is not None else np.zeros_like(e_impl)
        bound = REFEREE_FACTOR * e_ref + REFEREE_FLOOR
        bad = np.flatnonzero(~(e_impl < bound))                       # NaN fails
        c = int(np.argmax(np.where(np.isnan(e_impl), np.inf, e_impl / bound)))
        report[name] = (float(e_impl[c]), float(bound[c]))
        try:
            check_err("%s %s: worst channel %d of %d, vs float64 (float32 reference vs float64: %.3e)"
                      % (label, name, c, e_impl.size, e_ref[c]), e_impl[c], bound[c])
        except AssertionError as e:
            lines.append(str(e))
        if bad.size and failures is not None:
            failures[name] = bad
    if failures is None:
        assert not lines, "\n".join(lines)
    return report


def ref32(x, n, gamma, beta, eps, slope, addend, go, running, momentum, updates, device):
    """The float32 reference: the plain tensor expression (mean(0), var(0, unbiased=False), rsqrt, leaky_relu, autograd)
    over the first n >= 2 rows, on `device`. Not nn.BatchNorm1d. Returns the dict `compare` takes, n-row tensors."""
    import torch

    def t(a, grad=False):
        return torch.as_tensor(np.ascontiguousarray(a, np.float32)).to(device).requires_grad_(grad)

    assert n >= 2
    xv, g, b = t(np.asarray(x)[:n], True), t(gamma, True), t(beta, True)
    ad = t(np.asarray(addend)[:n], True) if addend is not None else None
    mean, var = xv.mean(0), xv.var(0, unbiased=False)
    z = (xv - mean) * torch.rsqrt(var + eps) * g + b
    if ad is not None:
        z = z + ad
    y = torch.nn.functional.leaky_relu(z, slope)
    grads = torch.autograd.grad(y, [xv, g, b] + ([ad] if ad is not None else []), t(np.asarray(go)[:n]))
    out = {"y": y, "dx": grads[0], "dgamma": grads[1], "dbeta": grads[2], "d_addend": grads[3] if ad is not None else None,
           "mean": mean, "var": var}
    if running is not None:
        rm, rv = t(running[0]), t(running[1])
        with torch.no_grad():
            for _ in range(updates):
                rm = (1 - momentum) * rm + momentum * mean
                rv = (1 - momentum) * rv + momentum * (var * (n / (n - 1)))
        out["running_mean"], out["running_var"] = rm, rv
    return {k: (v.detach().cpu().numpy() if v is not None else None) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------- case table

Case = collections.namedtuple("Case", "R D n family slope join variant seed", defaults=(0.1, False, "plain", 0))
# variant: "plain"; "misaligned" (the GPU test starts x, addend and go one float past a 16-byte boundary: the
# register-resident shape on the two-stage kernels); "large_mean" (x = randn * 2 + 60, |mean| = 30 sigma: the regime the
# shift exists for)

CASES = (
    # bn_small_* (R <= 128): one workgroup per 64 channels
    Case(128, 64, 128, "small"), Case(128, 64, 128, "small", 1.0), Case(128, 64, 128, "small", 0.1, True),
    Case(50, 66, 37, "small"), Case(50, 66, 37, "small", 0.1, True),            # D % 64, D % 4 != 0, padded rows
    Case(97, 200, 97, "small"),                                                  # four channel groups, ragged last of 8
    Case(2, 64, 2, "small"),                                                     # dx cancels
    Case(5, 64, 1, "small"),                                                     # variance 0
    Case(50, 66, 37, "small", 0.1, False, "large_mean"),
    # bn_mid_* (129..1024 rows, D % 4 == 0, aligned): rows in registers
    Case(129, 64, 129, "mid"),                                                   # one thread with a second row
    Case(1024, 16, 1024, "mid"), Case(1024, 16, 1024, "mid", 1.0), Case(1024, 16, 1024, "mid", 0.1, True),
    Case(600, 36, 577, "mid"), Case(600, 36, 577, "mid", 0.1, True),            # D % 16 != 0: last workgroup holds one quad
    Case(257, 128, 256, "mid"),                                                  # n on a 256-row boundary, one padded row
    Case(600, 36, 577, "mid", 0.1, False, "large_mean"),
    # two-stage (bn_stats_partial / bn_finish_apply, bn_bwd_reduce / bn_bwd_finish_apply)
    Case(1025, 64, 1025, "two"), Case(1025, 64, 1025, "two", 0.1, True),        # 17 row blocks, last of one row
    Case(300, 66, 263, "two"), Case(300, 66, 263, "two", 0.1, True),            # D % 4 != 0 above 128 rows
    Case(300, 64, 263, "two", 0.1, False, "misaligned"), Case(300, 64, 263, "two", 0.1, True, "misaligned"),
    Case(3137, 64, 3100, "two"),                                                 # 50 row blocks: four-per-trip loop
    Case(8300, 32, 8200, "two"), Case(8300, 32, 8200, "two", 1.0),              # > BN_FUSED_GY row groups: capped grid
    Case(300, 66, 263, "two", 0.1, True, "large_mean"),
)


def case_id(c):
    return "%s-%dx%d-n%d-s%g%s%s" % (c.family, c.R, c.D, c.n, c.slope, "-join" if c.join else "",
                                     "" if c.variant == "plain" else "-" + c.variant)


def inputs(c):
    """x, gamma, beta, go, addend (None without the join) of a case: float32, seeded by the case itself. Row 0 is an
    ordinary sample; rows >= n are ordinary samples too (the kernels must not read them into anything)."""
    rng = np.random.default_rng([c.R, c.D, c.n, int(c.slope * 10), int(c.join), len(c.variant), c.seed])
    f = np.float32
    x = (rng.standard_normal((c.R, c.D)) * 2 + (60 if c.variant == "large_mean" else 3)).astype(f)
    gamma = rng.uniform(0.5, 1.5, c.D).astype(f)
    beta = rng.uniform(-0.5, 0.5, c.D).astype(f)
    go = rng.standard_normal((c.R, c.D)).astype(f)
    addend = rng.standard_normal((c.R, c.D)).astype(f) if c.join else None
    return {"x": x, "gamma": gamma, "beta": beta, "go": go, "addend": addend}


def RUNNING0(D):
    """The running statistics of a fresh nn.BatchNorm1d."""
    return np.zeros(D, np.float32), np.ones(D, np.float32)


def oracle_of_case(c, inp, updates=2):
    """y_impl -> Oracle for a case's inputs, the running statistics moved `updates` times from a fresh module's."""
    return lambda y_impl: oracle(inp["x"], c.n, inp["gamma"], inp["beta"], EPS, c.slope, inp["addend"], inp["go"], y_impl,
                                 RUNNING0(c.D), MOMENTUM, updates)


def ref32_of_case(c, inp, device, updates=2):
    if c.n < 2:
        return None
    return ref32(inp["x"], c.n, inp["gamma"], inp["beta"], EPS, c.slope, inp["addend"], inp["go"], RUNNING0(c.D), MOMENTUM,
                 updates, device)
