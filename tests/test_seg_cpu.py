"""CPU: the float64 restatement of the segmentation loss / metrics contract (tests/seg_ref.py) against torch's own
formulation, the new entry points of the library, the drop-in's mvpnet.models.loss / metric import paths, and the
meter's host face. No GPU."""
import ctypes
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seg_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SEG_EXPORTS = ("mvk_seg_workspace_floats", "mvk_seg_loss_fwd", "mvk_seg_loss_fwd_f64", "mvk_seg_loss_bwd",
               "mvk_seg_loss_bwd_f64")

# (shape, ignore_index): 3-D and 4-D logits; ignore_index far outside, at 255 and inside [0, C)
CASES = [((2, 5, 65), -100), ((3, 20, 257), 255), ((2, 4, 5, 7), 2), ((1, 7, 33), -100), ((2, 6, 3, 4), 255)]


def torch_formulation(x, labels, w, ignore_index, scale):
    """F.cross_entropy on CPU float64 tensors. Labels outside [0, C) that are not ignore_index are masked to ignore_index
    first (CPU torch raises IndexError on them)."""
    C = x.shape[1]
    xt = torch.from_numpy(np.asarray(x, np.float64)).requires_grad_(True)
    lt = torch.from_numpy(labels.copy())
    lt[((lt < 0) | (lt >= C)) & (lt != ignore_index)] = ignore_index
    wt = None if w is None else torch.from_numpy(np.asarray(w, np.float64))
    loss = F.cross_entropy(xt, lt, weight=wt, ignore_index=ignore_index)
    (g,) = torch.autograd.grad(loss * scale, xt)
    return float(loss.detach()), g.numpy(), lt


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("shape,ignore_index", CASES)
def test_restatement_agrees_with_torch_cross_entropy(shape, ignore_index, weighted):
    x, labels, w = seg_ref.quantised_case(shape, seed=sum(shape) + int(weighted), ignore_index=ignore_index)
    labels.reshape(-1)[:2] = (shape[1], -5)                                            # two labels outside [0, C)
    w = w if weighted else None
    scale = 1.7
    ref = seg_ref.seg_reference(x, labels, w, ignore_index, grad_scale=scale)
    loss, grad, _ = torch_formulation(x, labels, w, ignore_index, scale)
    n, c = labels.size, shape[1]
    # both sides are float64 evaluations of the same sums: (8 + C + 2 N) roundings of 2^-53 on values <= max(1, |x| + log C)
    bound = seg_ref.loss_bound(n, c, 2.0 + math.log(c))
    assert ref["bad"] and abs(ref["loss"] - loss) <= bound, (ref["loss"], loss, bound)
    k_max = scale * (1.5 if weighted else 1.0) / ref["weight_sum"]                      # largest g w / W of any point
    assert np.abs(ref["grad"] - grad).max() <= seg_ref.loss_bound(n, c, 1.0) * k_max
    assert np.all(ref["grad"][np.broadcast_to(~np.expand_dims(ref["kept"], 1), ref["grad"].shape)] == 0.0)


def test_restatement_every_point_ignored_is_nan_like_torch():
    x, labels, w = seg_ref.quantised_case((2, 5, 9), seed=1)
    labels[:] = -100
    ref = seg_ref.seg_reference(x, labels, w, -100)
    loss, grad, _ = torch_formulation(x, labels, w, -100, 1.0)
    assert math.isnan(ref["loss"]) and math.isnan(loss)
    assert np.all(ref["grad"] == 0.0) and np.all(grad == 0.0)
    assert ref["counts"].tolist() == [0, 0] and not ref["conf"].any() and not ref["bad"]


@pytest.mark.parametrize("shape,ignore_index", CASES)
def test_restatement_counts_equal_argmax_mask_bincount(shape, ignore_index):
    """The reference's metric arithmetic (argmax(1), the ignore mask, eq / sum, bincount of n * label + pred) on CPU
    against the restatement, on logits quantised to multiples of 0.5 so that equal maxima are frequent."""
    x, labels, _ = seg_ref.quantised_case(shape, seed=7 + sum(shape), ignore_index=ignore_index)
    C = shape[1]
    xs = np.sort(x.reshape(shape[0], C, -1), axis=1)
    assert C == 1 or (xs[:, -1, :] == xs[:, -2, :]).any(), "the case has no tie between maximal classes"
    ref = seg_ref.seg_reference(x, labels, None, ignore_index)
    xt, lt = torch.from_numpy(x), torch.from_numpy(labels)
    pred = xt.argmax(1)
    assert np.array_equal(ref["pred"], pred.numpy())
    mask = lt != ignore_index
    lab_k, pred_k = lt[mask], pred[mask]
    tp = pred_k.eq(lab_k)
    assert ref["counts"].tolist() == [int(tp.sum()), tp.numel()]
    conf = torch.bincount(C * lab_k + pred_k, minlength=C * C).reshape(C, C)
    assert np.array_equal(ref["conf"], conf.numpy())


def test_library_exports_the_seg_entry_points_at_abi_9():
    import mvkpconv
    lib_mod = mvkpconv.sub("_lib")
    raw = ctypes.CDLL(lib_mod.LIB_PATH)
    header = open(mvkpconv._ROOT + "/include/mvkpconv.h").read()
    for name in SEG_EXPORTS:
        assert name in lib_mod.EXPORTS and hasattr(raw, name) and (" " + name + "(") in header, name
    assert lib_mod.ABI_VERSION == 9 and lib_mod.lib().mvk_abi_version() == 9
    assert "#define MVK_ABI_VERSION 9" in header
    lib = lib_mod.lib()
    assert lib.mvk_seg_workspace_floats(0) == 2 and lib.mvk_seg_workspace_floats(256) == 2
    assert lib.mvk_seg_workspace_floats(257) == 4
    # sizes and null operands are refused before anything is launched
    assert lib.mvk_seg_loss_fwd(None, 1, 257, 4, None, 1, -100, None, None, None, None, None, None, None, None) != 0
    assert b"bad sizes" in lib.mvk_last_error()
    assert lib.mvk_seg_loss_fwd(None, 1, 0, 4, None, 1, -100, None, None, None, None, None, None, None, None) != 0
    assert lib.mvk_seg_loss_bwd(None, 1, 257, 4, None, 1, -100, None, None, None, None, None, None) != 0
    assert lib.mvk_seg_loss_fwd_f64(None, 1, 5, 4, None, 1, -100, None, None, None, None, None, None, None, None) != 0
    assert lib.mvk_seg_loss_bwd_f64(None, 1, 5, 4, None, 1, -100, None, None, None, None, None, None) != 0
    assert b"null operand" in lib.mvk_last_error()


def test_wrappers_refuse_cpu_tensors_and_too_many_classes():
    import mvkpconv
    ops = mvkpconv.sub("ops")
    x, lab = torch.zeros(2, 5, 7), torch.zeros(2, 7, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.seg_loss(x, lab)
    with pytest.raises(RuntimeError, match="HBM"):
        ops.seg_stats(x, lab)
    with pytest.raises(RuntimeError, match="C = 257"):
        ops.seg_loss(torch.zeros(1, 257, 3), torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="C = 257"):
        ops.seg_stats(torch.zeros(1, 257, 3), torch.zeros(1, 3, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="labels"):
        ops.seg_loss(x, lab.float())
    with pytest.raises(RuntimeError, match="expected"):
        ops.seg_loss(x, torch.zeros(2, 8, dtype=torch.int64))


_CFG = ("class _T:\n"
        "    LABEL_WEIGHTS_PATH = ''\n"
        "class cfg:\n"
        "    TRAIN = _T\n")

_PN2 = ("net = PN2SSG(4, 5, sa_channels=((8, 8),), num_centroids=(4,), radius=(0.2,), max_neighbors=(4,),\n"
        "             fp_channels=((8,),), fp_neighbors=(3,), seg_channels=(8,))\n")


def _run(prog, cwd):
    return subprocess.run([sys.executable, "-c", prog], cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          text=True, timeout=300)


def test_loss_and_metric_imports_resolve_to_the_drop_in_without_a_reference_tree(tmp_path):
    """dropin/ first on sys.path and NO reference tree behind it: mvpnet.models.loss / metric are drop-in files, and
    PN2SSG.get_loss / get_metric (their lazy imports) build the drop-in's classes."""
    import mvkpconv
    dropin = os.path.join(ROOT, mvkpconv.PKG_NAME, "dropin")
    prog = (
        "import sys\n"
        "sys.path.insert(0, %r)\n"
        "from mvpnet.models.loss import SegLoss\n"
        "from mvpnet.models.metric import SegAccuracy, SegIoU\n"
        "from mvpnet.models.pn2.pn2ssg import PN2SSG\n"
        "for f in (SegLoss, SegAccuracy, SegIoU, PN2SSG):\n"
        "    assert 'dropin' in sys.modules[f.__module__].__file__, f\n"
        + _CFG + _PN2 +
        "loss = net.get_loss(cfg)\n"
        "assert type(loss) is SegLoss and loss.weight is None and loss.ignore_index == -100\n"
        "train, val = net.get_metric(cfg)\n"
        "for ms in (train, val):\n"
        "    assert type(ms[0]) is SegAccuracy and type(ms[1]) is SegIoU and ms[1].num_classes == 5 and ms[1].mat is None\n"
        "    assert (ms[0].name, ms[1].name) == ('seg_acc', 'seg_iou')\n"
        "assert train[0] is not val[0]\n"
        "print('SEG IMPORTS OK')\n") % (dropin,)
    r = _run(prog, tmp_path)
    assert r.returncode == 0 and "SEG IMPORTS OK" in r.stdout, r.stderr[-3000:]


def test_drop_in_loss_and_metric_win_over_a_tree_behind(tmp_path):
    """A stub tree (own text) behind the drop-in whose mvpnet/models/loss.py and metric.py raise on import: the drop-in's
    files come first, while another module of the same package still falls through to the tree."""
    import mvkpconv
    stub = {
        "mvpnet/__init__.py": "",
        "mvpnet/models/__init__.py": "",
        "mvpnet/models/loss.py": "raise ImportError('the tree behind must be shadowed by the drop-in')\n",
        "mvpnet/models/metric.py": "raise ImportError('the tree behind must be shadowed by the drop-in')\n",
        "mvpnet/models/other.py": "MARK = 'stub other'\n",
    }
    for rel, text in stub.items():
        f = tmp_path / rel
        f.parent.mkdir(parents=True, exist_ok=True)
        f.write_text(text)
    dropin = os.path.join(ROOT, mvkpconv.PKG_NAME, "dropin")
    prog = (
        "import sys\n"
        "sys.path.insert(0, %r); sys.path.append(%r)\n"
        "from mvpnet.models.loss import SegLoss\n"
        "from mvpnet.models.metric import SegAccuracy, SegIoU\n"
        "import mvpnet.models.other as O\n"
        "assert O.MARK == 'stub other'\n"
        "for f in (SegLoss, SegAccuracy, SegIoU):\n"
        "    assert 'dropin' in sys.modules[f.__module__].__file__, f\n"
        "print('SEG SHADOW OK')\n") % (dropin, str(tmp_path))
    r = _run(prog, tmp_path)
    assert r.returncode == 0 and "SEG SHADOW OK" in r.stdout, r.stderr[-3000:]


def _metric():
    import mvkpconv
    return mvkpconv.sub("dropin.mvpnet.models.metric")


def test_meter_host_face():
    """The reference meter's behaviour on values given from the host: format strings '{avg:.4f} ({global_avg:.4f})' and
    '{global_avg:.4f}', a window of the last 20 updates, NaN at count 0, reset."""
    m = _metric().SegAccuracy()
    assert m.name == "seg_acc" and m.ignore_index == -100
    assert m.fmt == "{avg:.4f} ({global_avg:.4f})" and m.summary_fmt == "{global_avg:.4f}"
    assert m.count == 0 and m.sum == 0.0 and math.isnan(m.global_avg) and math.isnan(m.avg)
    assert m.summary_str == "nan" and len(m.values) == 0 and m.values.maxlen == 20 and m.counts.maxlen == 20
    for i in range(25):
        m.update(i, 100)                                  # hits, points
    assert m.sum == sum(range(25)) and m.count == 2500
    assert list(m.values) == list(range(5, 25)) and list(m.counts) == [100] * 20
    avg, glob = sum(range(5, 25)) / 2000.0, sum(range(25)) / 2500.0
    assert m.avg == avg and m.global_avg == glob
    assert str(m) == "{avg:.4f} ({global_avg:.4f})".format(avg=avg, global_avg=glob)
    assert m.summary_str == "{global_avg:.4f}".format(global_avg=glob)
    m.update(3)                                           # count defaults to 1
    assert m.count == 2501 and list(m.counts)[-1] == 1
    m.reset()
    assert m.count == 0 and m.sum == 0.0 and len(m.values) == 0 and len(m.counts) == 0 and math.isnan(m.global_avg)


def test_iou_host_face():
    metric = _metric()
    iou = metric.SegIoU(3, ignore_index=255)
    assert iou.name == "seg_iou" and iou.num_classes == 3 and iou.ignore_index == 255 and iou.mat is None
    iou.mat = torch.tensor([[4, 1, 0], [2, 3, 0], [0, 0, 5]])
    want = np.array([4 / 7.0, 3 / 6.0, 1.0])
    assert np.allclose(iou.iou.numpy(), want, rtol=1e-6)
    assert abs(iou.global_avg - want.mean()) < 1e-6
    assert str(iou) == "{iou:.4f}".format(iou=want.mean()) and iou.summary_str == str(iou)
    iou.reset()
    assert iou.mat is None
    with pytest.raises(ValueError, match="num_classes"):
        iou.update_dict({"seg_logit": torch.zeros(1, 4, 2)}, {"seg_label": torch.zeros(1, 2, dtype=torch.int64)})
