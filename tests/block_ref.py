"""The cases of tests/block_cases.py through oracle/torch_port.py (_Net, forward, loss_fn) on the CPU in a given dtype.
What the oracle computes is not touched: torch_port.F is wrapped for the duration of a run by a recorder that keeps the
input of every leaky_relu and every batch_norm and calls the real function. From the records come the running
statistics after one training forward (momentum update with the unbiased variance, in the run's dtype) and the values
tests/test_blocks_cpu.py looks at for kinks. Results are numpy arrays; the float64 and float32 runs are cached."""
import collections
import functools

import numpy as np
import torch

import block_cases as bc
from oracle import torch_port

PREFIX = "blk"


class _Recorder:
    """Stands in for torch.nn.functional inside oracle/torch_port.py."""

    def __init__(self, real, names):
        self._real = real
        self._names = names             # id(BatchNorm weight tensor of the state dict) -> its name
        self.lrelu = []                 # inputs of leaky_relu, in call order
        self.bn = []                    # (state-dict prefix of the BatchNorm, input, running mean and variance before, momentum)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def leaky_relu(self, x, *a, **k):
        self.lrelu.append(x.detach().clone())
        return self._real.leaky_relu(x, *a, **k)

    def batch_norm(self, x, rm, rv, weight, *a, **k):
        name = self._names[id(weight)]
        self.bn.append((name[:-len("weight")], x.detach().clone(), rm.clone(), rv.clone(), a[2]))
        return self._real.batch_norm(x, rm, rv, weight, *a, **k)


class _recording:
    def __init__(self, sd):
        self.rec = _Recorder(torch_port.F, {id(t): n for n, t in sd.items() if n.endswith("batch_norm.weight")})

    def __enter__(self):
        self.old, torch_port.F = torch_port.F, self.rec
        return self.rec

    def __exit__(self, *exc):
        torch_port.F = self.old


def _trainable(name):
    return not name.endswith(("kernel_points", "running_mean", "running_var", "num_batches_tracked"))


def _state_tensors(state, dtype, prefix, grad):
    sd, leaves = {}, {}
    for n, v in state.items():
        t = torch.from_numpy(np.array(v))
        if t.is_floating_point():
            t = t.to(dtype)
            if grad and _trainable(n):
                leaves[n] = t.requires_grad_(True)
        sd[prefix + n] = t
    return sd, leaves


def _running(rec, strip):
    """{state-dict name: value after one training forward} from the recorded BatchNorm inputs."""
    out = {}
    for prefix, x, rm, rv, m in rec.bn:
        assert prefix.startswith(strip)
        p = prefix[len(strip):]
        assert p + "running_mean" not in out, "a BatchNorm ran twice"
        out[p + "running_mean"] = ((1 - m) * rm + m * x.mean(0)).numpy()
        out[p + "running_var"] = ((1 - m) * rv + m * x.var(0, unbiased=True)).numpy()
    return out


# tensors: {label: array} of everything the GPU test compares (y, dx, "grad <name>", running statistics by state-dict name,
#   min_d2 / deformed_KP for deformable blocks, "y eval"); kinks: the LeakyReLU inputs in call order;
# d_ext: |neighbour - deformed kernel point| / extent [Nq, H, K] of a deformable block, real: idx < Ns; extra: free-form
Result = collections.namedtuple("Result", "tensors kinks d_ext real extra")


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a))
    return t.to(dtype) if dtype is not None else t


def run_block(base, dtype):
    """One training forward + backward of the scalar sum(y go) [+ ALIAS_C sum(x) for a strided block: the second consumer of
    the block input] and one eval-mode forward."""
    c, i = bc.BY_NAME[base], bc.make_inputs(base)
    cfg = bc.config(c.use_bn, c.mod)
    strided = "strided" in c.block
    idx = _t(i.idx).long()
    batch = {"points": [_t(i.s, dtype), _t(i.q, dtype)] if strided else [_t(i.s, dtype)], "neighbors": [idx], "pools": [idx]}
    sd, leaves = _state_tensors(i.state, dtype, PREFIX + ".", True)
    x = _t(i.x, dtype).requires_grad_(True)
    go = _t(i.go, dtype)
    with _recording(sd) as rec:
        net = torch_port._Net(sd, cfg, True)
        y = net.block(c.block, PREFIX, x, batch, 0, bc.R)
    scalar = (y * go).sum()
    if strided:
        scalar = scalar + bc.ALIAS_C * x.sum()
    names = list(leaves)
    grads = torch.autograd.grad(scalar, [x] + [leaves[n] for n in names])
    out = {"y": y.detach().numpy(), "dx": grads[0].numpy()}
    for n, g in zip(names, grads[1:]):
        out["grad " + n] = g.numpy()
    out.update(_running(rec, PREFIX + "."))
    d_ext = real = None
    if "deform" in c.block:
        (min_d2, dkp, extent), = net.reg_terms
        out["min_d2"], out["deformed_KP"] = min_d2.detach().numpy(), dkp.detach().numpy()
        sp = torch.cat([batch["points"][0], torch.full((1, 3), 1e6, dtype=dtype)])
        rel = sp[idx] - batch["points"][-1][:, None, :]
        d_ext = ((rel[:, :, None, :] - dkp.detach()[:, None, :, :]) ** 2).sum(-1).sqrt().numpy() / extent
        real = i.idx < c.N
    with torch.no_grad():
        sd_eval, _ = _state_tensors(i.state, dtype, PREFIX + ".", False)
        out["y eval"] = torch_port._Net(sd_eval, cfg, False).block(c.block, PREFIX, _t(i.x, dtype), batch, 0, bc.R).numpy()
    return Result(out, [z.numpy() for z in rec.lrelu], d_ext, real, {})


def run_net(dtype, seed=bc.NET_SEED):
    """The two-level network of block_cases: logits, loss and every parameter gradient of torch_port.forward + loss_fn
    (labels renumbered like the product's lookup table: raw 0 is ignored, l -> l - 1), the eval-mode logits, and in
    `extra` the features the strided block's max-pool reads with its pool rows."""
    i = bc.make_net_inputs(seed)
    cfg = bc.config(architecture=bc.NET_ARCH)
    batch = {"points": [_t(p, dtype) for p in i.points], "neighbors": [_t(a).long() for a in i.neighbors],
             "pools": [_t(a).long() for a in i.pools], "upsamples": [_t(a).long() for a in i.upsamples],
             "features": _t(i.features, dtype)}
    labels = _t(i.labels) - 1
    sd, leaves = _state_tensors(i.state, dtype, "", True)
    trace = {}
    with _recording(sd) as rec:
        logits, reg = torch_port.forward(sd, cfg, batch, None, True, trace)
        loss = torch_port.loss_fn(logits, labels, reg, cfg)
    names = list(leaves)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    out = {"logits": logits.detach().numpy(), "loss": loss.detach().numpy().reshape(1)}
    for n, g in zip(names, grads):
        out["grad " + n] = g.numpy()
    out.update(_running(rec, ""))
    with torch.no_grad():
        sd_eval, _ = _state_tensors(i.state, dtype, "", False)
        out["y eval"] = torch_port.forward(sd_eval, cfg, batch, None, False)[0].numpy()
    pooled = trace["encoder_blocks.%d" % (bc.NET_ARCH.index("resnetb_strided") - 1)].detach().numpy()
    return Result(out, [z.numpy() for z in rec.lrelu], None, None, {"pooled_features": pooled, "pool_rows": i.pools[0]})


@functools.lru_cache(maxsize=None)
def block64(base):
    return run_block(base, torch.float64)


@functools.lru_cache(maxsize=None)
def block32(base):
    return run_block(base, torch.float32)


@functools.lru_cache(maxsize=None)
def net64():
    return run_net(torch.float64)


@functools.lru_cache(maxsize=None)
def net32():
    return run_net(torch.float32)


# ---------------------------------------------------------------- the conditions on the inputs (tests/test_blocks_cpu.py)

E_REF_MAX = 5e-6      # every compared tensor: L2-relative distance of the float32 run from the float64 run
MARGIN = 10.0         # 3 (what referee_check grants the HIP path over the reference's own error) x ~3 (max-abs against L2)


def l2(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def live_rows(base):
    """Rows of a deformable case with a real neighbour: min_d2 of the others is the distance to the shadow point (3e12)
    and is compared on its own."""
    i = bc.make_inputs(base)
    return (i.idx < i.s.shape[0]).any(1)


def reference_errors(r64, r32, base=None):
    """{label: e_ref} over the compared tensors (min_d2: the live rows; the shadow-only rows separately)."""
    out = {}
    for k, v in r64.tensors.items():
        if k == "min_d2":
            live = live_rows(base)
            out[k] = l2(r32.tensors[k][live], v[live])
            out[k + " (shadow rows)"] = l2(r32.tensors[k][~live], v[~live])
        else:
            out[k] = l2(r32.tensors[k], v)
    return out


def kink_margins(r64, r32):
    """[(min |z64|, max |z32 - z64|)] per recorded LeakyReLU input."""
    assert len(r64.kinks) == len(r32.kinks) and r64.kinks
    return [(float(np.abs(a).min()), float(np.abs(b.astype(np.float64) - a).max())) for a, b in zip(r64.kinks, r32.kinks)]


def max_pool_gap(features, rows):
    """Smallest gap between the largest and the second-largest candidate of any (row, channel) of a max-pool over
    `rows` (the zero shadow row takes part once, however often a row names it)."""
    ns = features.shape[0]
    fp = np.concatenate([features, np.zeros((1, features.shape[1]), features.dtype)]).astype(np.float64)
    vals = fp[rows]                                                        # [Nq, H, C]
    dup = (rows >= ns) & (np.cumsum(rows >= ns, axis=1) > 1)
    vals = np.where(dup[:, :, None], -np.inf, vals)
    top = np.sort(vals, axis=1)[:, -2:, :]
    return float((top[:, 1] - top[:, 0]).min())


def deform_band(r64, r32):
    """(entries of real neighbours inside the kink band of the linear influence and of the in-range filter, the band's
    half width): |d / extent - 1| < MARGIN x the float32 run's largest deviation of d / extent."""
    dev = float(np.abs(r32.d_ext.astype(np.float64) - r64.d_ext)[r64.real].max())
    inside = (np.abs(r64.d_ext - 1) < MARGIN * dev) & r64.real[:, :, None]
    return int(inside.sum()), MARGIN * dev


def deform_argmin_ties(r64, r32):
    """Number of (row, kernel point) whose two closest real neighbours are closer to each other in d / extent than
    MARGIN x the float32 run's largest deviation (rows with fewer than two real neighbours cannot tie)."""
    dev = float(np.abs(r32.d_ext.astype(np.float64) - r64.d_ext)[r64.real].max())
    d = np.where(r64.real[:, :, None], r64.d_ext, np.inf)
    two = np.sort(d, axis=1)[:, :2, :]
    with np.errstate(invalid="ignore"):          # (inf - inf: a row of shadow entries only)
        gap = two[:, 1] - two[:, 0]
    return int((gap[np.isfinite(gap)] < MARGIN * dev).sum())


def conditions(r64, r32, base=None):
    """Everything test_blocks_cpu.py asserts, as a list of the violations (empty: the seed is good)."""
    bad = []
    for k, e in reference_errors(r64, r32, base).items():
        if not e <= E_REF_MAX:
            bad.append("e_ref %s %.3e" % (k, e))
    for n, (lo, dev) in enumerate(kink_margins(r64, r32)):
        if not lo >= MARGIN * dev:
            bad.append("kink %d: min |z| %.3e < %g x %.3e" % (n, lo, MARGIN, dev))
    if r64.d_ext is not None:
        n, w = deform_band(r64, r32)
        if n:
            bad.append("%d neighbour / kernel point pairs within %.2e of the extent" % (n, w))
        n = deform_argmin_ties(r64, r32)
        if n:
            bad.append("%d tied min_d2 arg-mins" % n)
        if not np.array_equal(r64.d_ext < 1, r32.d_ext < 1):
            bad.append("float32 and float64 disagree on the in-range filter")
    if "pooled_features" in r64.extra:
        f64, f32 = r64.extra["pooled_features"], r32.extra["pooled_features"]
        dev = float(np.abs(f32.astype(np.float64) - f64).max())
        gap = max_pool_gap(f64, r64.extra["pool_rows"])
        if not gap >= MARGIN * dev:
            bad.append("max-pool gap %.3e < %g x %.3e" % (gap, MARGIN, dev))
    return bad
