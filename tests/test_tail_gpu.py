"""The tail of a training step on the HIP kernels -- ops.cross_entropy_lut (csrc/loss.hip, xent_*) and optim.FusedClipSGD
(csrc/optim.hip) -- against the float64 restatement of tests/tail_ref.py over its case tables (validated against torch
float64 in tests/test_tail_cpu.py). The referee is the float32 run of the reference's own formulation (torch on the
CPU: CrossEntropyLoss(weight, ignore_index=-1) on the renumbered labels; clip_grad_value_ + torch.optim.SGD) with the
project's factor and floor (tests/util.py).

Loss, per case: |loss - f64| <= 3 |torch32 - f64| + 1e-5 |f64|; the gradient as a whole tensor through referee_check; the
gradient row by row, max_c |dx - dx64| over the row's own scale g w_t / sum w, the worst row held to 3 x the same
figure of torch32 + 8 * 2^-24 (two device transcendentals of <= 2 ulp, one division, one product); ignored rows exactly
zero; two runs bit-equal; NaN and an all-zero gradient when no point is kept; NaN where the reference has NaN when every
kept point has weight 0.
Optimiser, after each of 6 steps, per parameter and per momentum buffer: max|hip - f64| <= 3 max|torch32 - f64| +
4 * 2^-24 max|f64| (one rounding of the stored value, with room); which tensors take the float4 path is asserted from
the pointers. clip_in_place, step(only=...) and non-finite gradients are compared bit for bit.

Measured on the MI355X (every figure is in the parity log through check_err), e_hip against e_ref = torch32's own distance:
  loss           |HIP - f64| at most 7.2e-4 (n16641-c13-big, logits of 1e4: a loss of ~1.6e4, torch32 1.2e-3); at the usual
                 scale at most 2.7e-6 on a loss of ~6 (n16384-c20, torch32 3.1e-7). Largest e_hip / e_ref: 11.8 (n257-c2,
                 3.3e-7 against 2.8e-8), 8.7 (n16384-c20), 7.3 (n257-c255), 5.2 (n16385-c13-g0), all others below 3: each of
                 them a few float32 roundings of the value and far inside the 1e-5 |f64| floor (the kernel adds 256 points
                 per workgroup and the workgroup sums one after the other in float32, torch sums in blocks).
  dlogits, L2    e_hip 1.6e-8 .. 1.4e-7 against e_ref 1.6e-8 .. 1.6e-7; largest ratio 2.6 (n16641-c13-big), bound 1.0e-5.
  dlogits, row   worst row over its own scale: e_hip at most 1.32e-6 (n16385-c256, torch32 1.41e-6, bound 4.7e-6); largest
                 e_hip / e_ref 1.44 (n255-c20), 1.34, 1.33, 1.30: no row stands out and the factor of 3 is not approached;
                 the 8 * 2^-24 floor alone decides only the cases whose gradient is exactly zero (C = 1, g = 0, n64-c2-ninf).
  optimiser      max|HIP - f64| per tensor: parameters 2.5e-7 .. 9.4e-7, momentum 3.0e-8 .. 6.2e-7, in 20 of 24 columns the
                 same figure as torch32 to four digits; the worst tensor of every case sits at 0.21 .. 0.25 of its bound.
  joint head     W 6.2e-8 (torch32 6.2e-8), b 3.8e-8 (3.8e-8), the five losses 8.8e-8 (9.0e-8), bound 1.0e-5.
Before the clamp of csrc/optim.hip kept NaN and optim.py passed inf, the four non-finite cases failed (a NaN gradient became
-clip, +-inf became +-3e38 with clipping off) and everything else passed."""
import importlib

import numpy as np
import pytest
import torch

import tail_ref as tr
from util import REFEREE_FACTOR, REFEREE_FLOOR, bits_equal, check_err, referee_check

pytestmark = pytest.mark.gpu

PKG = "enhancing-3d-point-cloud-segmentation-using-multi-modal-fusion-with-2d-images_amd"
ROW_FLOOR = 8 * tr.EPS32
SGD_FLOOR = 4 * tr.EPS32


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return importlib.import_module(PKG + ".ops")


@pytest.fixture(scope="module")
def optim():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return importlib.import_module(PKG + ".optim")


def T(a):
    return torch.from_numpy(np.array(a)).cuda()          # (a copy: the cached inputs are read-only)


def N(t):
    return t.detach().cpu().numpy()


def at_most(bound):
    """check_err asserts err < bound; the bounds here are <=."""
    return np.nextafter(np.float64(bound), np.inf)


# ---------------------------------------------------------------------------------------------------------- the loss

def _torch32_xent(i, C):
    x = torch.from_numpy(np.array(i["logits"])).requires_grad_(True)
    target = torch.from_numpy(tr.classes_of(i["labels"], i["lut"], C))
    w = None if i["weight"] is None else torch.from_numpy(np.array(i["weight"]))
    loss = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1)(x.t().unsqueeze(0), target.unsqueeze(0))
    (dx,) = torch.autograd.grad(loss * i["g"], x)
    return float(loss.detach()), dx.numpy()


def _hip_xent(ops, i, lut=None):
    x = T(i["logits"]).requires_grad_(True)
    w = None if i["weight"] is None else T(i["weight"])
    loss = ops.cross_entropy_lut(x, T(i["labels"]), T(i["lut"] if lut is None else lut), w)
    (dx,) = torch.autograd.grad(loss * i["g"], x)
    return N(loss), N(dx)


@pytest.mark.parametrize("name", [c["name"] for c in tr.XENT_CASES])
def test_cross_entropy_lut_vs_float64(ops, name):
    c, i = tr.XENT_BY_NAME[name], tr.xent_inputs(name)
    loss64, dx64, kept = tr.xent_expected(name)
    loss, dx = _hip_xent(ops, i)
    assert loss.dtype == np.float32 and dx.dtype == np.float32 and dx.shape == dx64.shape
    # ignored rows, reproducibility, no kept point
    assert (dx[~kept] == 0).all()
    loss_b, dx_b = _hip_xent(ops, i)
    assert bits_equal(loss, loss_b) and bits_equal(dx, dx_b)
    loss_n, dx_n = _hip_xent(ops, i, lut=np.full_like(i["lut"], -1))
    assert np.isnan(loss_n) and (dx_n == 0).all()
    if c["weights"] == "zeroall":                    # 0 / 0: NaN where the reference has NaN, zero in the ignored rows
        assert np.isnan(loss64) and np.isnan(loss)
        assert np.array_equal(np.isnan(dx), np.isnan(dx64)) and np.isnan(dx[kept]).all()
        return
    assert np.isfinite(loss64) and np.isfinite(dx64).all() and np.isfinite(dx).all()
    loss32, dx32 = _torch32_xent(i, c["C"])
    check_err("xent %s loss: |HIP - f64| (torch32: %.3e)" % (name, abs(loss32 - loss64)), abs(float(loss) - loss64),
              at_most(REFEREE_FACTOR * abs(loss32 - loss64) + REFEREE_FLOOR * abs(loss64)))
    referee_check("xent %s dlogits" % name, dx, dx32, dx64)
    scale = tr.row_scale(i["labels"], i["lut"], i["weight"], i["g"], c["C"])
    r_hip, r_ref = tr.worst_row(dx, dx64, scale), tr.worst_row(dx32, dx64, scale)
    check_err("xent %s dlogits worst row / its scale (torch32: %.3e)" % (name, r_ref), r_hip,
              at_most(REFEREE_FACTOR * r_ref + ROW_FLOOR))


def test_cross_entropy_lut_refuses_more_than_256_classes(ops):
    x = torch.zeros(4, tr.XC_MAX + 1, device="cuda", requires_grad=True)
    labels = torch.zeros(4, dtype=torch.int64, device="cuda")
    lut = torch.tensor([-1, 0, -1], dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="xent: bad sizes"):
        ops.cross_entropy_lut(x, labels, lut)
    with pytest.raises(RuntimeError):
        ops.cross_entropy_lut(x[:, :5], labels, lut[:2])
    torch.cuda.synchronize()                         # nothing was launched that could fail later
    loss = ops.cross_entropy_lut(x[:, :tr.XC_MAX].contiguous(), labels, lut)
    assert float(loss.detach()) == pytest.approx(np.log(256.0), rel=1e-6)


# ------------------------------------------------------------------------------------------------------ the optimiser

def _torch32_sgd_trajectory(params, grads, momentum, clip_value):
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(a))) for a in params]
    opt = torch.optim.SGD([dict(params=ps[:5], **tr.SGD_GROUPS[0]), dict(params=ps[5:], **tr.SGD_GROUPS[1])], lr=1.0,
                          momentum=momentum)
    clip = tr.effective_clip(clip_value)
    out = []
    for row in grads:
        for p, g in zip(ps, row):
            p.grad = None if g is None else torch.from_numpy(np.array(g))
        if clip is not None:
            torch.nn.utils.clip_grad_value_(ps, clip)
        opt.step()
        out.append(([p.detach().numpy().copy() for p in ps],
                    [opt.state[p]["momentum_buffer"].numpy().copy() if "momentum_buffer" in opt.state[p] else None for p in ps]))
    return out


def _fused(optim, params, momentum, clip_value, clip_in_place=False):
    ps = [torch.nn.Parameter(T(a)) for a in params]
    opt = optim.FusedClipSGD([dict(params=ps[:5], **tr.SGD_GROUPS[0]), dict(params=ps[5:], **tr.SGD_GROUPS[1])], lr=1.0,
                             momentum=momentum, clip_value=clip_value, clip_in_place=clip_in_place)
    assert opt._chunk == tr.SGD_CHUNK                # the lengths 4095 .. 8193 of the table sit on this seam
    return ps, opt


def _set_grads(ps, row, offset=()):
    for p, g in zip(ps, row):
        if g is None:
            p.grad = None
        elif p.numel() in offset:                    # a float32 view one element into its storage
            buf = torch.empty(p.numel() + 1, device="cuda")
            view = buf[1:].view(p.shape)
            view.copy_(T(g))
            assert view.storage_offset() == 1 and view.is_contiguous() and view.data_ptr() % 16 == 4
            p.grad = view
        else:
            p.grad = T(g)


def _vec_lengths(ps, opt):
    """The tensors whose three pointers are 16-byte aligned (csrc/optim.hip takes the float4 path for them)."""
    return {p.numel() for p in ps if p.grad is not None and p.numel() >= 4
            and (p.data_ptr() | p.grad.data_ptr() | opt.state[p]["momentum_buffer"].data_ptr()) % 16 == 0}


def _state(ps, opt):
    return [N(p) for p in ps], [N(opt.state[p]["momentum_buffer"]) for p in ps]


@pytest.mark.parametrize("name", [c["name"] for c in tr.SGD_CASES])
def test_fused_clip_sgd_vs_float64(optim, name):
    c = tr.SGD_BY_NAME[name]
    params, grads = tr.sgd_inputs(c["order"])
    want = tr.sgd_expected(name)
    ref = _torch32_sgd_trajectory(params, grads, c["momentum"], c["clip_value"])
    ps, opt = _fused(optim, params, c["momentum"], c["clip_value"])
    worst = {"p": (0.0, 0.0, 0.0), "m": (0.0, 0.0, 0.0)}          # (e_hip / bound, e_hip, e_ref) of the worst tensor
    for step, row in enumerate(grads):
        _set_grads(ps, row, c["offset_grad"])
        if step == 0:
            assert _vec_lengths(ps, opt) == tr.sgd_vec_lengths(c)
        ptrs = [None if p.grad is None else p.grad.data_ptr() for p in ps]
        opt.step()
        assert ptrs == [None if p.grad is None else p.grad.data_ptr() for p in ps]        # no copy was substituted
        got = _state(ps, opt)
        for kind, g_all, w_all, r_all in (("p", got[0], want[step][0], ref[step][0]), ("m", got[1], want[step][1], ref[step][1])):
            for k, (g, w) in enumerate(zip(g_all, w_all)):
                e_hip = float(np.abs(g.astype(np.float64) - w).max())
                e_ref = 0.0 if r_all[k] is None else float(np.abs(r_all[k].astype(np.float64) - w).max())
                bound = REFEREE_FACTOR * e_ref + SGD_FLOOR * float(np.abs(w).max())
                assert e_hip <= bound, "%s step %d %s[%d] (n = %d): %.3e > %.3e (torch32 %.3e)" % (
                    name, step, kind, k, g.size, e_hip, bound, e_ref)
                if bound > 0 and e_hip / bound >= worst[kind][0]:
                    worst[kind] = (e_hip / bound, e_hip, e_ref)
    for kind in ("p", "m"):
        check_err("sgd %s %s: worst max|HIP - f64| / bound over 6 steps (there HIP %.3e, torch32 %.3e)"
                  % (name, kind, worst[kind][1], worst[kind][2]), worst[kind][0], at_most(1.0))


@pytest.mark.parametrize("order", ["mis", "al_a"])
def test_fused_clip_sgd_clip_in_place(optim, order):
    """clip_in_place=True leaves the bits of torch.clamp(g, -clip, clip) in .grad, False leaves .grad alone; the step
    itself is the same."""
    params, grads = tr.sgd_inputs(order)
    row = grads[1]                                   # scale 1.0: most elements beyond the bound
    states = []
    for in_place in (True, False):
        ps, opt = _fused(optim, params, tr.F(0.9), 0.5, clip_in_place=in_place)
        _set_grads(ps, row)
        opt.step()
        for p, g in zip(ps, row):
            want = np.clip(g, np.float32(-0.5), np.float32(0.5)) if in_place else g
            assert bits_equal(N(p.grad), want)
            assert not in_place or bits_equal(N(p.grad), torch.clamp(torch.from_numpy(np.array(g)), -0.5, 0.5).numpy())
        states.append(_state(ps, opt))
    assert all(bits_equal(a, b) for x, y in zip(*states) for a, b in zip(x, y))


@pytest.mark.parametrize("split", ["even-odd", "none-all", "all-none", "groups"])
def test_fused_clip_sgd_step_only_partition(optim, split):
    """step(only=A) then step(only=B) over a partition of the parameters = one step(), bit for bit, over two steps the
    second of which has a parameter without a gradient (in A or in B, by the split)."""
    params, grads = tr.sgd_inputs("al_a")
    whole_ps, whole = _fused(optim, params, tr.F(0.9), 0.5)
    part_ps, part = _fused(optim, params, tr.F(0.9), 0.5)
    n = len(params)
    A = {"even-odd": list(range(0, n, 2)), "none-all": [], "all-none": list(range(n)), "groups": list(range(5))}[split]
    B = [k for k in range(n) if k not in A]
    for step in (1, 2):
        _set_grads(whole_ps, grads[step])
        _set_grads(part_ps, grads[step])
        whole.step()
        part.step(only=[part_ps[k] for k in A])
        part.step(only=(part_ps[k] for k in B))
        assert any(p.grad is None for p in part_ps) == (step == 2)
        for a, b in zip(_state(whole_ps, whole), _state(part_ps, part)):
            assert all(bits_equal(x, y) for x, y in zip(a, b))
    assert not bits_equal(N(whole_ps[2]), params[2])


def _non_finite_rows(order):
    """(row with NaN at element 0, +inf in the middle, -inf at the end of every tensor of 3 elements or more; its finite
    twin with 0, +0.5, -0.5 there; the positions per tensor)."""
    _, grads = tr.sgd_inputs(order)
    bad, twin, pos = [], [], []
    for g in grads[1]:
        b, t = np.array(g), np.array(g)
        n = g.size
        where = (0, n // 2, n - 1) if n >= 3 else ()
        for j, (vb, vt) in zip(where, ((np.nan, 0.0), (np.inf, 0.5), (-np.inf, -0.5))):
            b.reshape(-1)[j], t.reshape(-1)[j] = vb, vt
        bad.append(b), twin.append(t), pos.append(where)
    return bad, twin, pos


@pytest.mark.parametrize("order", ["mis", "al_a"])
@pytest.mark.parametrize("clip_value", [0.5, None])
def test_fused_clip_sgd_non_finite_gradients(optim, order, clip_value):
    """A NaN gradient is a NaN parameter and momentum (clip_grad_value_ and torch.clamp keep a NaN), an infinite one moves
    the parameter by the bound when clipping is on and stays infinite when it is off, and nothing else changes: every other
    element has the bits of the step with finite gradients there. Scalar path ("mis") and float4 path ("al_a")."""
    params, grads = tr.sgd_inputs(order)
    bad, twin, pos = _non_finite_rows(order)
    rows = {"bad": [grads[0], bad, grads[2]], "twin": [grads[0], twin, grads[2]]}
    out = {}
    for key, seq in rows.items():
        ps, opt = _fused(optim, params, tr.F(0.9), clip_value)
        for step, row in enumerate(seq):
            _set_grads(ps, row)
            if step == 1:
                vec = _vec_lengths(ps, opt)
                assert vec == (set() if order == "mis" else tr.sgd_vec_lengths({"order": order, "offset_grad": ()}))
            opt.step()
            if step == 1:
                out[key] = _state(ps, opt)
        out[key + "-end"] = _state(ps, opt)
    ref = _torch32_sgd_trajectory(params, rows["bad"], tr.F(0.9), clip_value)
    for stage, r in (("", ref[1]), ("-end", ref[2])):
        for kind in (0, 1):
            for k, where in enumerate(pos):
                got, fin = (out[key + stage][kind][k].reshape(-1) for key in ("bad", "twin"))
                want = r[kind][k].reshape(-1)
                assert np.isfinite(fin).all()
                label = "%s %s[%d]" % (stage or "step", "pm"[kind], k)
                # non-finite exactly where torch's float32 run is, with the same NaN / +inf / -inf
                assert np.array_equal(np.isnan(got), np.isnan(want)), label
                assert np.array_equal(np.isposinf(got), np.isposinf(want)) and np.array_equal(np.isneginf(got), np.isneginf(want)), label
                exempt = np.zeros(got.shape, bool)
                if where:
                    assert np.isnan(got[where[0]]), label
                    exempt[where[0]] = True
                    if clip_value is None:
                        # the step itself: p = -+inf, m = +-inf. One step on, weight decay makes them inf - inf = NaN, in
                        # torch as here (the comparison above)
                        if not stage:
                            assert np.isinf(got[where[1]]) and np.isinf(got[where[2]]) and got[where[1]] == -got[where[2]], label
                        assert not np.isfinite(got[list(where[1:])]).any(), label
                        exempt[list(where[1:])] = True
                # everything else -- with clipping on, the infinite positions too: they moved by exactly the bound
                assert bits_equal(got[~exempt], fin[~exempt]), label
                assert np.isfinite(got[~exempt]).all(), label


# ------------------------------------------------------------------------------------------------------ the joint head

def test_head_loss_and_optimiser_chain_vs_float64(ops, optim):
    """linear_bias_lrelu -> cross_entropy_lut (times g) -> backward -> FusedClipSGD.step, 5 steps on a 300 x 16 -> 7 head:
    the weights after step 5 against the same chain in float64, refereed by the chain in torch float32."""
    h, i = tr.HEAD, tr.head_inputs()
    W64, b64, losses64, _ = tr.head_trajectory64()

    def run(dev, layer, loss_of, make_opt, before_step):
        W = torch.nn.Parameter(torch.from_numpy(np.array(i["W"])).to(dev))
        b = torch.nn.Parameter(torch.from_numpy(np.array(i["b"])).to(dev))
        opt, losses = make_opt([W, b]), []
        for x, lab in zip(i["xs"], i["labels"]):
            opt.zero_grad()
            loss = loss_of(layer(torch.from_numpy(x).to(dev), W, b), lab)
            (loss * h["g"]).backward()
            before_step([W, b])
            opt.step()
            losses.append(float(loss.detach()))
        return N(W), N(b), losses

    lut, weight = T(i["lut"]), T(i["weight"])
    hip = run("cuda", lambda x, W, b: ops.linear_bias_lrelu(x, W, b, h["slope"]),
              lambda y, lab: ops.cross_entropy_lut(y, T(lab), lut, weight),
              lambda ps: optim.FusedClipSGD(ps, lr=h["lr"], momentum=h["momentum"], weight_decay=h["weight_decay"],
                                            clip_value=h["clip_value"]), lambda ps: None)
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(np.array(i["weight"])), ignore_index=-1)
    ref = run("cpu", lambda x, W, b: torch.nn.functional.leaky_relu(x @ W.t() + b, h["slope"]),
              lambda y, lab: crit(y.t().unsqueeze(0), torch.from_numpy(tr.classes_of(lab, i["lut"], h["classes"])).unsqueeze(0)),
              lambda ps: torch.optim.SGD(ps, lr=h["lr"], momentum=h["momentum"], weight_decay=h["weight_decay"]),
              lambda ps: torch.nn.utils.clip_grad_value_(ps, h["clip_value"]))
    failures = []
    referee_check("head chain W after 5 steps", hip[0], ref[0], W64, failures=failures)
    referee_check("head chain b after 5 steps", hip[1], ref[1], b64, failures=failures)
    referee_check("head chain losses of the 5 steps", hip[2], ref[2], losses64, failures=failures)
    assert not failures, "\n".join(failures)
    assert np.abs(W64 - i["W"]).max() > 10 * h["lr"] * h["clip_value"] / 4          # the weights moved
