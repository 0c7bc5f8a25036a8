"""tests/tail_ref.py validated without a GPU: each float64 oracle against torch in float64 (the reference's own
formulation: labels outside the valid set -> -1, CrossEntropyLoss(weight, ignore_index=-1) on the (1, C, N) logits;
clip_grad_value_ + torch.optim.SGD), NaN and inf where torch has them, and the conditions on the case tables that keep
the GPU comparison from passing on an empty set."""
import numpy as np
import pytest
import torch

import tail_ref as tr

REL = 1e-12


def _close(a, b, label):
    """Same non-finite positions and values; the finite rest within REL of the tensor's largest finite magnitude."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape, label
    fin = np.isfinite(b)
    assert np.array_equal(np.isfinite(a), fin), label + ": non-finite positions differ"
    assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~fin & ~np.isnan(b)], b[~fin & ~np.isnan(b)]), label
    if fin.any():
        err = np.abs(a[fin] - b[fin]).max()
        assert err <= REL * max(np.abs(b[fin]).max(), 1e-300), "%s: %.3e" % (label, err)


def _torch_xent(i, C, dtype):
    x = torch.from_numpy(np.array(i["logits"])).to(dtype).requires_grad_(True)
    target = torch.from_numpy(tr.classes_of(i["labels"], i["lut"], C))
    w = None if i["weight"] is None else torch.from_numpy(np.array(i["weight"])).to(dtype)
    loss = torch.nn.CrossEntropyLoss(weight=w, ignore_index=-1)(x.t().unsqueeze(0), target.unsqueeze(0))
    (dx,) = torch.autograd.grad(loss * i["g"], x)
    return loss.detach().numpy(), dx.numpy()


@pytest.mark.parametrize("name", [c["name"] for c in tr.XENT_CASES])
def test_xent64_equals_torch_float64(name):
    c, i = tr.XENT_BY_NAME[name], tr.xent_inputs(name)
    loss, dx, kept = tr.xent_expected(name)
    ref_loss, ref_dx = _torch_xent(i, c["C"], torch.float64)
    _close(loss, ref_loss, name + " loss")
    _close(dx, ref_dx, name + " dlogits")
    # per row, against the row's own scale (a max-norm over the tensor hides a row of a small class weight)
    scale = tr.row_scale(i["labels"], i["lut"], i["weight"], i["g"], c["C"])
    assert tr.worst_row(dx, ref_dx, scale) <= 1e-12
    assert np.array_equal(kept, tr.classes_of(i["labels"], i["lut"], c["C"]) >= 0)
    assert (dx[~kept] == 0).all()
    assert np.isnan(loss) == (c["weights"] == "zeroall")


@pytest.mark.parametrize("name", [c["name"] for c in tr.XENT_CASES])
def test_xent_case_is_what_it_says(name):
    """The table conditions: enough kept points, every class present, and each special input really there."""
    c, i = tr.XENT_BY_NAME[name], tr.xent_inputs(name)
    N, C = c["N"], c["C"]
    x, labels, lut = i["logits"], i["labels"], i["lut"]
    assert x.shape == (N, C) and x.dtype == np.float32 and labels.shape == (N,)
    assert labels.dtype == (np.int64 if c["i64"] else np.int32) and lut.dtype == np.int32 and lut.shape[0] >= 3
    t = tr.classes_of(labels, lut, C)
    kept = t >= 0
    assert 3 * kept.sum() >= N
    if N >= 4 * C and c["weights"] != "zeroall":
        assert np.array_equal(np.unique(t[kept]), np.arange(C))
    if N >= 8:                                       # the out-of-table labels, through both ends of the table
        top = lut.shape[0] - 3
        assert list(labels[:3]) == [-5, -1, top + 1] and int(labels[3]) == (2 ** 40 if c["i64"] else 2 ** 31 - 1)
        assert (t[:2] == (0 if c["lut"] == "ends" else -1)).all()
        assert (t[2:4] == {"ends": C - 1, "len3": C - 1}.get(c["lut"], -1)).all()
        assert (~kept).any() or c["lut"] == "len3"
    if c["lut"] == "edge":
        raw = np.asarray(lut[1:-1])
        assert (raw == C).sum() == 1 and (raw == C + 1).sum() == 1
        hit = np.isin(labels, np.flatnonzero((lut == C) | (lut == C + 1)) - 1)
        assert hit.any() and (t[hit] == -1).all()
    if c["lut"] == "len3":
        assert lut.shape[0] == 3
    if c["scale"] == "shift":                        # exp of the raw logit overflows float32, in every row
        assert (x.max(axis=1) > 89.0).mean() > 0.99  # float32 exp overflows above 88.73
    if c["scale"] == "ninf":
        assert (np.isneginf(x).sum(axis=1) == 1).all() and np.isfinite(x[np.arange(N), np.where(kept, t, 0)])[kept].all()
    if c["scale"] == "const":
        assert (x == x[:, :1]).all()
    if c["weights"] in ("zero1", "zeroall"):
        z = np.flatnonzero(i["weight"] == 0)
        assert z.shape[0] == 1 and (t == z[0]).any()
        assert ((t[kept] == z[0]).all()) == (c["weights"] == "zeroall")
    elif i["weight"] is not None:
        assert (i["weight"] >= 0.5).all() and (i["weight"] < 1.5).all()


def test_xent64_no_kept_point_and_table_ends():
    x = np.random.default_rng(0).standard_normal((5, 4)).astype(np.float32)
    lut = np.array([-1, 0, 4, 5, 3, -1], np.int32)                        # raw 1 -> 4 and raw 2 -> 5: not classes of C = 4
    loss, dx, kept = tr.xent64(x, np.array([-7, 1, 2, 4, 2 ** 40]), lut, None, 1.0)
    assert np.isnan(loss) and not kept.any() and (dx == 0).all()
    lut[0], lut[-1] = 2, 1
    assert list(tr.classes_of(np.array([-7, -1, 0, 1, 2, 3, 4, 5, 2 ** 40]), lut, 4)) == [2, 2, 0, -1, -1, 3, 1, 1, 1]


# ------------------------------------------------------------------------------------------------------ the optimiser

def _torch_sgd_trajectory(params, grads, momentum, clip_value, dtype):
    ps = [torch.nn.Parameter(torch.from_numpy(np.array(a)).to(dtype)) for a in params]
    groups = [dict(params=ps[:5], **tr.SGD_GROUPS[0]), dict(params=ps[5:], **tr.SGD_GROUPS[1])]
    opt = torch.optim.SGD(groups, lr=1.0, momentum=momentum)
    clip = tr.effective_clip(clip_value)
    out = []
    for row in grads:
        for p, g in zip(ps, row):
            p.grad = None if g is None else torch.from_numpy(np.array(g)).to(dtype)
        if clip is not None:
            torch.nn.utils.clip_grad_value_(ps, clip)
        opt.step()
        out.append(([p.detach().numpy().copy() for p in ps],
                    [opt.state[p]["momentum_buffer"].numpy().copy() if "momentum_buffer" in opt.state[p] else None for p in ps]))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in tr.SGD_CASES])
def test_clip_sgd64_equals_torch_float64(name):
    c = tr.SGD_BY_NAME[name]
    params, grads = tr.sgd_inputs(c["order"])
    ref = _torch_sgd_trajectory(params, grads, c["momentum"], c["clip_value"], torch.float64)
    for step, ((p, m), (rp, rm)) in enumerate(zip(tr.sgd_expected(name), ref)):
        for k in range(len(p)):
            _close(p[k], rp[k], "%s step %d p[%d]" % (name, step, k))
            if rm[k] is not None:                     # torch keeps no buffer with momentum 0 (ours then holds d)
                _close(m[k], rm[k], "%s step %d m[%d]" % (name, step, k))


@pytest.mark.parametrize("name", [c["name"] for c in tr.SGD_CASES])
def test_sgd_case_is_what_it_says(name):
    c = tr.SGD_BY_NAME[name]
    lens = tr.SGD_ORDERS[c["order"]]
    assert sorted(lens) == sorted(tr.SGD_LENGTHS)
    params, grads = tr.sgd_inputs(c["order"])
    assert [a.shape for a in params] == [tr.SGD_SHAPES[n] for n in lens] and len(grads) == tr.SGD_STEPS == 6
    assert [k for row in grads for k, g in enumerate(row) if g is None] == [lens.index(tr.SGD_NO_GRAD[1])]
    # the bound of 0.5 cuts between 5 % and 95 % of the gradient elements on EVERY step (so clipping on differs from
    # clipping off on every step), more on the odd ones
    share = []
    for row in grads:
        flat = np.concatenate([g.reshape(-1) for g in row if g is not None])
        share.append(float((np.abs(flat) > 0.5).mean()))
        assert 0.05 < share[-1] < 0.95
    assert all(share[s] < 0.2 < 0.5 < share[s + 1] for s in range(0, 6, 2))
    if tr.effective_clip(c["clip_value"]) is None:
        assert c["clip_value"] in (None, 0.0, -1.0)
        on = tr.sgd_trajectory64(params, grads, c["momentum"], 0.5)
        assert all(np.abs(a - b).max() > 1e-4 for a, b in zip(on[-1][0], tr.sgd_expected(name)[-1][0]) if a.size >= 4095)
    # alignment by order
    vec = tr.sgd_vec_lengths(c)
    if c["order"] == "mis":
        assert lens[0] == 1 and vec == set()
    else:
        assert vec and all(n % 4 == 0 or n > 4 for n in vec)


def test_sgd_orders_cover_both_paths_for_every_tensor():
    al = [tr.sgd_vec_lengths({"order": o, "offset_grad": ()}) for o in ("al_a", "al_b")]
    assert al[0] | al[1] == {n for n in tr.SGD_LENGTHS if n >= 4}
    assert {4096, tr.BIG, 4} <= al[0] & al[1]
    off = set().union(*(c["offset_grad"] for c in tr.SGD_CASES))
    assert off and all(any(n in tr.sgd_vec_lengths(dict(c, offset_grad=())) for c in tr.SGD_CASES if n in c["offset_grad"])
                       for n in off)                     # an offset gradient sits on a tensor that is otherwise aligned
    assert {c["momentum"] for c in tr.SGD_CASES} == {0.0, tr.F(0.9), tr.F(0.98)}
    assert {c["clip_value"] for c in tr.SGD_CASES} == {0.5, None, 0.0, -1.0}


def test_clamp64_and_torch_keep_nan_and_leave_inf_alone_without_a_bound():
    g = np.array([np.nan, np.inf, -np.inf, 0.7, -0.7, 0.2], np.float32)
    want = np.array([np.nan, 0.5, -0.5, 0.5, -0.5, np.float32(0.2)], np.float64)
    got = tr.clamp64(g, 0.5)
    assert np.array_equal(got, want, equal_nan=True)
    assert np.array_equal(tr.clamp64(g, None), g.astype(np.float64), equal_nan=True)
    assert np.array_equal(torch.clamp(torch.from_numpy(g), -0.5, 0.5).numpy(), want.astype(np.float32), equal_nan=True)
    p = torch.nn.Parameter(torch.zeros(6))
    p.grad = torch.from_numpy(g.copy())
    torch.nn.utils.clip_grad_value_([p], 0.5)
    assert np.array_equal(p.grad.numpy(), want.astype(np.float32), equal_nan=True)
    # one step of the oracle and of torch float64 on these gradients, with and without the bound
    for clip in (0.5, None):
        q = torch.nn.Parameter(torch.ones(6, dtype=torch.float64))
        q.grad = torch.from_numpy(g.astype(np.float64))
        if clip is not None:
            torch.nn.utils.clip_grad_value_([q], clip)
        opt = torch.optim.SGD([q], lr=0.1, momentum=0.9, weight_decay=1e-3)
        opt.step()
        p64, m64 = tr.clip_sgd64(np.ones(6), g, np.zeros(6), 0.1, 1e-3, 0.9, clip)
        _close(p64, q.detach().numpy(), "p clip %s" % clip)
        _close(m64, opt.state[q]["momentum_buffer"].numpy(), "m clip %s" % clip)
        assert np.isnan(p64[0]) and (np.isinf(p64[1:3]).all() if clip is None else np.isfinite(p64[1:]).all())


# ------------------------------------------------------------------------------------------------------ the joint head

def test_head_trajectory64_equals_torch_float64_and_stays_off_the_kink():
    h, i = tr.HEAD, tr.head_inputs()
    W64, b64, losses, margin = tr.head_trajectory64()
    W = torch.nn.Parameter(torch.from_numpy(i["W"]).double())
    b = torch.nn.Parameter(torch.from_numpy(i["b"]).double())
    opt = torch.optim.SGD([W, b], lr=h["lr"], momentum=h["momentum"], weight_decay=h["weight_decay"])
    crit = torch.nn.CrossEntropyLoss(weight=torch.from_numpy(i["weight"]).double(), ignore_index=-1)
    clipped = 0.0
    for step, (x, lab) in enumerate(zip(i["xs"], i["labels"])):
        y = torch.nn.functional.leaky_relu(torch.from_numpy(x).double() @ W.t() + b, h["slope"])
        target = torch.from_numpy(tr.classes_of(lab, i["lut"], h["classes"]))
        assert 3 * int((target >= 0).sum()) >= h["rows"]
        loss = crit(y.t().unsqueeze(0), target.unsqueeze(0))
        opt.zero_grad()
        (loss * h["g"]).backward()
        clipped = max(clipped, float((W.grad.abs() > h["clip_value"]).double().mean()))
        torch.nn.utils.clip_grad_value_([W, b], h["clip_value"])
        opt.step()
        assert abs(losses[step] - loss.item()) <= REL * abs(loss.item())
    _close(W64, W.detach().numpy(), "W")
    _close(b64, b.detach().numpy(), "b")
    assert 0.05 < clipped < 0.95
    # no pre-activation within reach of a float32 rounding of the LeakyReLU kink (|v| ~ 1: roundings of ~1e-7)
    assert margin > 1e-5
