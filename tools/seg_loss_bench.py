"""Development-only (GPU box): the tail of one MVPNet training step -- segmentation loss, both metric updates, the loss's
backward down to the logits' gradient -- fused (SegLoss / SegAccuracy / SegIoU of the drop-in on seg_fwd_k /
seg_bwd_k of csrc/loss.hip) against the torch formulation the drop-in fell through to before, written out below: one
F.cross_entropy, and per metric an argmax(1), the ignore mask, two mask indexings, then eq / sum / .item() for the
accuracy and bincount for the confusion.

Shapes: logits (B, 20, 8192) float32 with B = 32 (the reference configuration's batch of chunks) and B = 1; a tenth of
the labels ignored. Both paths compute the same loss, gradient, hit count and confusion (checked before timing).

Times: median [min .. max] milliseconds between two HIP events after a device synchronisation, 20 calls after 5 warm-ups,
the two paths alternating (DESIGN 7j's method). Launches: device kernels and memory copies of one call, counted with
torch.profiler. Writes profiles/seg_loss_bench.txt (or the path given).
usage: python tools/seg_loss_bench.py [out.txt] [calls]"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvkpconv

ops = mvkpconv.sub("ops")
loss_mod = mvkpconv.sub("dropin.mvpnet.models.loss")
metric = mvkpconv.sub("dropin.mvpnet.models.metric")
dev = torch.device("cuda:0")
CLASSES, POINTS, IGNORE = 20, 8192, -100


def pair_ms(fn_a, fn_b, calls, warmup=5):
    """Two callables timed alternately: ((median, min, max) of a, (median, min, max) of b)."""
    out = ([], [])
    for it in range(warmup + calls):
        for which, fn in enumerate((fn_a, fn_b)):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out[which].append(e0.elapsed_time(e1))
    return tuple((float(np.median(t)), float(np.min(t)), float(np.max(t))) for t in out)


def device_events(fn):
    """(kernels, memory copies / fills) the device ran for one call."""
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    from torch.autograd import DeviceType
    kernels = copies = 0
    for ev in prof.events():
        if ev.device_type == DeviceType.CUDA:
            if ev.name.startswith(("Memcpy", "Memset")):
                copies += 1
            else:
                kernels += 1
    return kernels, copies


class TorchTail:
    """The torch formulation of the tail: what mvpnet/models/loss.py and metric.py of a tree behind the drop-in compute."""

    def __init__(self):
        self.hits, self.points, self.mat = 0, 0, None

    def __call__(self, logits, labels):
        loss = F.cross_entropy(logits, labels, ignore_index=IGNORE)
        # accuracy
        pred = logits.argmax(1)
        mask = labels != IGNORE
        lab_k, pred_k = labels[mask], pred[mask]
        tp = pred_k.eq(lab_k)
        self.hits += tp.sum().item()
        self.points += tp.numel()
        # IoU
        pred = logits.argmax(1)
        mask = labels != IGNORE
        lab_k, pred_k = labels[mask], pred[mask]
        with torch.no_grad():
            if self.mat is None:
                self.mat = lab_k.new_zeros((CLASSES, CLASSES))
            self.mat += torch.bincount(CLASSES * lab_k + pred_k, minlength=CLASSES ** 2).reshape(CLASSES, CLASSES)
        loss.backward()
        return loss


class FusedTail:
    def __init__(self):
        self.loss = loss_mod.SegLoss(ignore_index=IGNORE)
        self.acc, self.iou = metric.SegAccuracy(ignore_index=IGNORE), metric.SegIoU(CLASSES, ignore_index=IGNORE)

    def __call__(self, logits, labels):
        preds, lab = {"seg_logit": logits}, {"seg_label": labels}
        loss = self.loss(preds, lab)["seg_loss"]
        self.acc.update_dict(preds, lab)
        self.iou.update_dict(preds, lab)
        loss.backward()
        return loss


class Lines(list):
    """The report's lines, shown as they come."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "seg_loss_bench.txt")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lines = Lines()
    lines.append("seg_loss_bench: loss + SegAccuracy.update_dict + SegIoU.update_dict + loss.backward() on (B, %d, %d) float32 "
                 "logits, a tenth of the labels ignored; median [min .. max] ms by HIP events, %d alternating calls after 5 "
                 "warm-ups" % (CLASSES, POINTS, calls))
    fmt = "%-22s torch %8.3f [%8.3f .. %8.3f]   fused %8.3f [%8.3f .. %8.3f]   fused / torch %6.3f"
    for b in (32, 1):
        torch.manual_seed(b)
        logits = (torch.randn(b, CLASSES, POINTS, device=dev) * 3).requires_grad_(True)
        labels = torch.randint(0, CLASSES, (b, POINTS), device=dev)
        labels[torch.rand(b, POINTS, device=dev) < 0.1] = IGNORE
        # the two paths agree
        tt, ft = TorchTail(), FusedTail()
        lt = tt(logits, labels)
        gt, logits.grad = logits.grad, None
        lf = ft(logits, labels)
        gf, logits.grad = logits.grad, None
        lt, lf = float(lt.detach()), float(lf.detach())
        assert abs(lt - lf) < 2e-6 * max(1.0, abs(lt))
        rel = float((gt - gf).abs().max() / gt.abs().max())
        assert rel < 1e-5 and torch.equal(tt.mat, ft.iou.mat) and (tt.hits, tt.points) == (ft.acc.sum, ft.acc.count)

        def run(tail):
            logits.grad = None
            tail(logits, labels)

        (tk, tc), (fk, fc) = device_events(lambda: run(tt)), device_events(lambda: run(ft))
        t_torch, t_fused = pair_ms(lambda: run(tt), lambda: run(ft), calls)
        lines.append(fmt % (("B = %2d x %d points" % (b, POINTS),) + t_torch + t_fused + (t_fused[0] / t_torch[0],)))
        lines.append("    device work per call: torch %d kernels + %d copies / fills, fused %d kernels + %d copies / fills; the "
                     "torch path waits for the device for the two mask sizes, .item() and bincount, the fused path not at all"
                     % (tk, tc, fk, fc))
        lines.append("    largest gradient difference relative to the largest gradient %.2e; fused max %s torch min"
                     % (rel, "<" if t_fused[2] < t_torch[1] else ">="))
        del logits, labels
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
