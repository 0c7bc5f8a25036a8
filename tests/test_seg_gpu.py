"""GPU: the fused segmentation loss / metrics kernel (csrc/loss.hip, seg_*) against the float64 restatement
(tests/seg_ref.py), and the drop-in's SegLoss / SegAccuracy / SegIoU against the reference's arithmetic written out with
torch ops on the same device tensors."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_ref
import util

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (B, C, *): smallest; wave edge with a batch boundary inside a wave; workgroup edge with several partials; the largest
# LDS histogram; the global-atomic confusion; XC_MAX; trailing dimensions
SHAPES = [(1, 1, 1), (2, 5, 63), (2, 5, 64), (2, 5, 65), (3, 20, 257), (2, 64, 300), (2, 65, 300), (1, 256, 70), (2, 4, 5, 7)]
SCALE = 1.7


def dropin(name):
    import mvkpconv
    return mvkpconv.sub(name)


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available(), "-m gpu tests need the MI355X"
    return dropin("ops")


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()              # a copy: the shared cases are read-only


_CASES = {}


def case(shape, ignore_index=-100):
    """(logits f32, labels i64, weights f32, references {weighted: ...}) of a shape, computed once and left unchanged."""
    key = (shape, ignore_index)
    if key not in _CASES:
        x, labels, w = seg_ref.quantised_case(shape, seed=11 + sum(shape), ignore_index=ignore_index)
        labels.reshape(-1)[0] = shape[1] - 1                                  # at least one kept point
        refs = {wd: seg_ref.seg_reference(x, labels, w if wd else None, ignore_index, grad_scale=SCALE) for wd in (False, True)}
        for a in (x, labels, w):
            a.setflags(write=False)
        _CASES[key] = (x, labels, w, refs)
    return _CASES[key]


def run(ops, x, labels, w, ignore_index=-100):
    xt = x.clone().requires_grad_(True)
    loss, (counts, conf) = ops.seg_loss(xt, labels, weight=w, ignore_index=ignore_index)
    (g,) = torch.autograd.grad(loss * SCALE, xt)
    return loss.detach(), g, counts, conf


def check_against(ref, shape, dtype, weighted, loss, g, counts, conf, label):
    n, c = int(np.prod(shape)) // shape[1], shape[1]
    got, want = float(loss), float(ref["loss"])
    if dtype == torch.float32:
        # the bounds test_cross_entropy_lut_vs_torch holds the same arithmetic to
        util.check_err(label + " loss", abs(got - want), 2e-6 * max(1.0, abs(want)))
        util.check_err(label + " grad", util.rel_err(g.cpu().numpy(), ref["grad"]), 1e-5)
    else:
        # two float64 evaluations of the same sums: (8 + C + 2 N) roundings of 2^-53 (seg_ref.loss_bound, as in the CPU test)
        assert abs(got - want) <= seg_ref.loss_bound(n, c, 2.0 + math.log(c)), (label, got, want)
        k_max = SCALE * (1.5 if weighted else 1.0) / ref["weight_sum"]
        assert np.abs(g.cpu().numpy() - ref["grad"]).max() <= seg_ref.loss_bound(n, c, 1.0) * k_max, label
    assert counts.dtype == torch.int64 and conf.dtype == torch.int64 and tuple(conf.shape) == (c, c)
    assert counts.cpu().tolist() == ref["counts"].tolist(), label
    assert np.array_equal(conf.cpu().numpy(), ref["conf"]), label


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
@pytest.mark.parametrize("i64", [False, True])
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_seg_loss_against_the_restatement(ops, shape, weighted, i64, dtype):
    x, labels, w, refs = case(shape)
    ref = refs[weighted]
    xs = np.sort(x.reshape(shape[0], shape[1], -1), axis=1)
    assert shape[1] == 1 or (xs[:, -1, :] == xs[:, -2, :]).any()             # equal maxima are in the case
    xt, lt = dev(x).to(dtype), dev(labels).to(torch.int64 if i64 else torch.int32)
    wt = dev(w).to(dtype) if weighted else None
    loss, g, counts, conf = run(ops, xt, lt, wt)
    label = "seg_loss %s w=%d i64=%d %s" % (shape, weighted, i64, str(dtype)[6:])
    assert loss.dtype == dtype and g.dtype == dtype and g.shape == xt.shape
    check_against(ref, shape, dtype, weighted, loss, g, counts, conf, label)
    assert np.all(g.cpu().numpy()[np.broadcast_to(~np.expand_dims(ref["kept"], 1), g.shape)] == 0.0)
    # run to run: bit equal
    loss2, g2, counts2, conf2 = run(ops, xt, lt, wt)
    assert torch.equal(loss, loss2) and torch.equal(g, g2) and torch.equal(counts, counts2) and torch.equal(conf, conf2)
    # the metrics-only launch, and the forms that save nothing
    c3, f3 = ops.seg_stats(xt, lt)
    assert torch.equal(c3, counts) and torch.equal(f3, conf)
    with torch.no_grad():
        loss4, (c4, f4) = ops.seg_loss(xt.clone().requires_grad_(True), lt, weight=wt)
        loss5 = ops.seg_loss(xt, lt, weight=wt, with_stats=False)
    assert torch.equal(loss4, loss) and torch.equal(loss5, loss) and torch.equal(c4, counts) and torch.equal(f4, conf)
    assert not loss4.requires_grad
    ops.seg_check_labels()                                                   # no label outside [0, C) was met


@pytest.mark.parametrize("ignore_index", [255, 2])
def test_ignore_index_at_255_and_inside_the_classes(ops, ignore_index):
    shape = (3, 20, 257)
    x, labels, w, refs = case(shape, ignore_index)
    assert (labels == ignore_index).sum() > labels.size // 4
    loss, g, counts, conf = run(ops, dev(x), dev(labels), dev(w), ignore_index)
    check_against(refs[True], shape, torch.float32, True, loss, g, counts, conf, "seg_loss ignore_index=%d" % ignore_index)
    if ignore_index == 2:
        assert not conf[2].any().item()                                      # the ignored class has no row
    c3, f3 = ops.seg_stats(dev(x), dev(labels), ignore_index=ignore_index)
    assert torch.equal(c3, counts) and torch.equal(f3, conf)
    ops.seg_check_labels()


def test_every_point_ignored(ops):
    x, labels, w, _ = case((2, 5, 65))
    lt = torch.full(labels.shape, -100, dtype=torch.int64, device="cuda")
    loss, g, counts, conf = run(ops, dev(x), lt, dev(w))
    assert torch.isnan(loss).item() and not g.any().item()
    assert counts.cpu().tolist() == [0, 0] and not conf.any().item()
    ops.seg_check_labels()


def test_labels_outside_the_classes_are_left_out_and_reported(ops):
    shape = (2, 5, 65)
    x, labels, w, _ = case(shape)
    labels = labels.copy()
    labels[0, 3], labels[1, 64] = shape[1], -5
    ref = seg_ref.seg_reference(x, labels, w, -100, grad_scale=SCALE)
    assert ref["bad"]
    ops.seg_check_labels()
    for i64 in (True, False):
        lt = dev(labels).to(torch.int64 if i64 else torch.int32)
        loss, g, counts, conf = run(ops, dev(x), lt, dev(w))
        check_against(ref, shape, torch.float32, True, loss, g, counts, conf, "seg_loss labels outside [0, C) i64=%d" % i64)
        assert not g[0, :, 3].any().item() and not g[1, :, 64].any().item()
        with pytest.raises(RuntimeError, match="outside"):
            ops.seg_check_labels()
        ops.seg_check_labels()                                               # cleared by the read
        ops.seg_stats(dev(x), lt)
        with pytest.raises(RuntimeError, match="outside"):
            ops.seg_check_labels()
        ops.seg_check_labels()


def test_non_contiguous_logits(ops):
    shape = (3, 20, 257)
    x, labels, w, _ = case(shape)
    xt, lt, wt = dev(x), dev(labels), dev(w)
    view = xt.transpose(1, 2).contiguous().transpose(1, 2)                   # (B, C, S) over (B, S, C) memory
    assert not view.is_contiguous() and torch.equal(view, xt)
    a, b = run(ops, xt, lt, wt), run(ops, view, lt, wt)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    assert all(torch.equal(u, v) for u, v in zip(ops.seg_stats(xt, lt), ops.seg_stats(view, lt)))


# ----------------------------------------------------------------------------------------------------------------------
# the modules
# ----------------------------------------------------------------------------------------------------------------------
N_CLS, IGN = 6, 255


def batches():
    out = []
    for i in range(3):
        x, labels, _ = seg_ref.quantised_case((2, N_CLS, 130 + i), seed=40 + i, ignore_index=IGN)
        out.append((dev(x), dev(labels)))
    return out


class Written:
    """The reference's metric arithmetic with torch ops (argmax(1), the ignore mask, eq / sum, bincount)."""

    def __init__(self):
        self.pairs, self.mat = [], torch.zeros((N_CLS, N_CLS), dtype=torch.int64, device="cuda")

    def update(self, x, labels):
        pred = x.argmax(1)
        mask = labels != IGN
        lab_k, pred_k = labels[mask], pred[mask]
        tp = pred_k.eq(lab_k)
        self.pairs.append((tp.sum().item(), tp.numel()))
        self.mat += torch.bincount(N_CLS * lab_k + pred_k, minlength=N_CLS ** 2).reshape(N_CLS, N_CLS)

    def check(self, acc, iou):
        hits, pts = sum(p[0] for p in self.pairs), sum(p[1] for p in self.pairs)
        assert torch.equal(iou.mat, self.mat) and iou.mat.is_cuda and iou.mat.dtype == torch.int64
        assert acc.sum == hits and acc.count == pts and acc.global_avg == hits / pts
        assert list(acc.values) == [p[0] for p in self.pairs] and list(acc.counts) == [p[1] for p in self.pairs]
        assert acc.avg == np.sum([p[0] for p in self.pairs]) / np.sum([p[1] for p in self.pairs])
        assert str(acc) == "{avg:.4f} ({global_avg:.4f})".format(avg=acc.avg, global_avg=hits / pts)
        h = self.mat.float()
        want = torch.diag(h) / (h.sum(1) + h.sum(0) - torch.diag(h))
        assert torch.equal(iou.iou, want) and iou.global_avg == want.mean().item()
        assert str(iou) == "{iou:.4f}".format(iou=want.mean().item()) and iou.summary_str == str(iou)


@pytest.mark.parametrize("with_loss", [True, False])
def test_modules_over_three_batches(ops, with_loss, monkeypatch):
    loss_mod, metric = dropin("dropin.mvpnet.models.loss"), dropin("dropin.mvpnet.models.metric")
    seg_loss = loss_mod.SegLoss(ignore_index=IGN)
    acc, iou, written = metric.SegAccuracy(ignore_index=IGN), metric.SegIoU(N_CLS, ignore_index=IGN), Written()
    calls = []
    real = ops.seg_stats
    monkeypatch.setattr(ops, "seg_stats", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    for x, labels in batches():
        preds, lab = {"seg_logit": x.clone().requires_grad_(True)}, {"seg_label": labels}
        if with_loss:
            out = seg_loss(preds, lab)
            assert set(out) == {"seg_loss"}
            want = F.cross_entropy(x, labels, ignore_index=IGN)
            assert abs(float(out["seg_loss"].detach()) - float(want)) < 2e-6 * max(1.0, abs(float(want)))
            out["seg_loss"].backward()
        acc.update_dict(preds, lab)
        iou.update_dict(preds, lab)
        written.update(x, labels)
    # with the loss in front no metrics launch at all; alone, one per batch (the second metric takes the first one's)
    assert len(calls) == (0 if with_loss else 3)
    written.check(acc, iou)
    acc.reset()
    iou.reset()
    assert iou.mat is None and acc.count == 0 and math.isnan(acc.global_avg)
    with pytest.raises(ValueError, match="num_classes"):
        metric.SegIoU(N_CLS + 1).update_dict({"seg_logit": batches()[0][0]}, {"seg_label": batches()[0][1]})


def test_stale_statistics_are_not_served(ops):
    loss_mod, metric = dropin("dropin.mvpnet.models.loss"), dropin("dropin.mvpnet.models.metric")
    x, labels = batches()[0]
    labels = labels.clone()
    preds, lab = {"seg_logit": x}, {"seg_label": labels}
    loss_mod.SegLoss(ignore_index=IGN)(preds, lab)
    labels[0, :40] = IGN                                                     # in place, after the loss
    labels[1, :40] = 1
    acc, iou, written = metric.SegAccuracy(ignore_index=IGN), metric.SegIoU(N_CLS, ignore_index=IGN), Written()
    acc.update_dict(preds, lab)
    iou.update_dict(preds, lab)
    written.update(x, labels)
    written.check(acc, iou)
    # another ignore_index is not served from the record either
    other = metric.SegAccuracy(ignore_index=0)
    other.update_dict(preds, lab)
    pred = x.argmax(1)
    mask = (labels != 0) & (labels != IGN)                                   # 255 is outside [0, C): left out, and reported
    assert other.count == int(mask.sum()) and other.sum == int((pred[mask] == labels[mask]).sum())
    with pytest.raises(RuntimeError, match="outside"):
        ops.seg_check_labels()


class _Train:
    LABEL_WEIGHTS_PATH = ""


class _Cfg:
    TRAIN = _Train


def test_pn2ssg_get_loss_gradients(ops, monkeypatch):
    """A one-level PN2SSG: the parameter gradients of get_loss(cfg)(preds, batch)['seg_loss'] against those of
    F.cross_entropy on the same logits of the same network, both measured against a float64 evaluation of the loss
    (the network referee's bound, util.referee_check)."""
    import mvkpconv
    before = set(sys.modules)
    monkeypatch.syspath_prepend(os.path.join(ROOT, mvkpconv.PKG_NAME, "dropin"))       # get_loss imports mvpnet.models.loss
    try:
        PN2SSG = dropin("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
        torch.manual_seed(5)
        net = PN2SSG(4, 5, sa_channels=((8, 8),), num_centroids=(4,), radius=(0.5,), max_neighbors=(4,),
                     fp_channels=((8,),), fp_neighbors=(3,), seg_channels=(8,), dropout_prob=0.0).cuda().train()
        rng = np.random.default_rng(5)
        batch = {"points": dev(rng.random((2, 3, 64)).astype(np.float32)),
                 "feature": dev(rng.standard_normal((2, 4, 64)).astype(np.float32)),
                 "seg_label": dev(rng.integers(0, 5, (2, 64)))}
        batch["seg_label"][0, :9] = -100
        seg_loss = net.get_loss(_Cfg)
        assert "dropin" in sys.modules[type(seg_loss).__module__].__file__
        train_metric, val_metric = net.get_metric(_Cfg)
        preds = net(batch)
        params = [p for p in net.parameters()]
        names = [n for n, _ in net.named_parameters()]
        seg_loss(preds, batch)["seg_loss"].backward(retain_graph=True)
        hip = [p.grad.clone() for p in params]                               # every parameter is reached
        logits = preds["seg_logit"]
        ref32 = torch.autograd.grad(F.cross_entropy(logits, batch["seg_label"]), params, retain_graph=True)
        x64 = logits.detach().double().requires_grad_(True)
        (d64,) = torch.autograd.grad(F.cross_entropy(x64, batch["seg_label"]), x64)
        f64 = torch.autograd.grad(logits, params, grad_outputs=d64.float())
        failures = []
        for name, a, b, c in zip(names, hip, ref32, f64):
            util.referee_check("PN2SSG get_loss grad " + name, a.cpu().numpy(), b.cpu().numpy(), c.cpu().numpy(), failures=failures)
        assert not failures, "\n".join(failures)
        for m in train_metric + val_metric:
            m.update_dict(preds, batch)
        mask = batch["seg_label"] != -100
        hits = int((logits.argmax(1)[mask] == batch["seg_label"][mask]).sum())
        assert train_metric[0].sum == hits and val_metric[0].count == int(mask.sum())
        assert int(train_metric[1].mat.sum()) == int(mask.sum())
    finally:
        for name in set(sys.modules) - before:                               # the top-level mirror packages of this test
            if name.split(".")[0] in ("mvpnet", "_native", "_fallthrough"):
                del sys.modules[name]


def test_no_host_wait_until_a_value_is_read(ops):
    loss_mod, metric = dropin("dropin.mvpnet.models.loss"), dropin("dropin.mvpnet.models.metric")
    seg_loss = loss_mod.SegLoss(ignore_index=IGN)
    acc, iou = metric.SegAccuracy(ignore_index=IGN), metric.SegIoU(N_CLS, ignore_index=IGN)
    bs = batches()

    def step(x, labels, with_loss):
        preds, lab = {"seg_logit": x.clone().requires_grad_(True)}, {"seg_label": labels}
        if with_loss:
            seg_loss(preds, lab)["seg_loss"].backward()
        acc.update_dict(preds, lab)
        iou.update_dict(preds, lab)

    step(*bs[0], True)                                                       # first use: allocations, the status word
    torch.cuda.synchronize()
    one = torch.ones(1, device="cuda")
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            one.item()
            honoured = False
        except RuntimeError:
            honoured = True
        if honoured:
            step(*bs[1], True)
            step(*bs[2], False)                                              # the metrics-only launch
            with pytest.raises(RuntimeError):
                acc.global_avg
            with pytest.raises(RuntimeError):
                iou.global_avg
    finally:
        torch.cuda.set_sync_debug_mode("default")
    if not honoured:
        pytest.skip("this torch build does not raise on .item() under set_sync_debug_mode('error')")
    assert acc.count > 0 and iou.global_avg > 0.0
