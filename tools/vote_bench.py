"""Development-only (GPU box): what test-time inference costs per batch on the headline workload's network (early
fusion, one ~19 k-point sphere of radius 1.2, three views) in eval mode under torch.no_grad():

  (i)   the forward as it was before freeze_inference (nn.BatchNorm1d + activation / join launches),
  (ii)  the forward after models.blocks.freeze_inference,
  (iii) the reference's route for one batch's vote: softmax(outputs).cpu().numpy(), points / indices to the host, the
        NumPy loop of utils/tester.py:160-186,
  (iv)  utils.tester.VoteAccumulator.update (csrc/vote.hip).

Median milliseconds over eager calls, each bracketed by HIP events after a device synchronisation (the host part of
(iii) falls between its two events: the stream idles while NumPy works). (i) is the baseline of (ii), (iii) of (iv).
Writes profiles/vote_bench.txt (or the path given).  usage: python tools/vote_bench.py [out.txt] [calls]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvkpconv

syn = mvkpconv.sub("synthetic")
blocks = mvkpconv.sub("dropin.models.blocks")
tester = mvkpconv.sub("dropin.utils.tester")
dev = torch.device("cuda:0")


def median_ms(fn, calls, warmup=5):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(calls):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "vote_bench.txt")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 30
    torch.manual_seed(0)
    np.random.seed(0)
    cfg = syn.make_config("early")
    sphere = syn.raw_sphere(seed=0, radius=cfg.in_radius)
    staged = syn.stage_spheres([sphere], dev, [syn.sphere_views(sphere, nv=3)])
    limits = syn.calibrate_limits(cfg, staged)
    batch, lens = syn.build_batch(cfg, staged, limits, torch.int32)
    n = lens[0]
    batch.input_inds = torch.arange(n, device=dev)             # the sphere is its whole cloud here
    batch.cloud_inds = torch.zeros(1, dtype=torch.int32, device=dev)
    net = syn.build_model(cfg, dev)
    net.eval()
    lines = ["vote_bench: early fusion, 1 sphere, N0 = %d points, %d classes, eval mode, no_grad; median [min .. max] ms of %d "
             "eager calls" % (n, cfg.num_classes, calls)]

    with torch.no_grad():
        fwd = lambda: net(batch, cfg)
        blocks.unfreeze_inference(net)
        t_unfrozen = median_ms(fwd, calls)
        blocks.freeze_inference(net)
        t_frozen = median_ms(fwd, calls)
        outputs = net(batch, cfg)

        smooth, ratio = 0.95, 0.7
        host_votes = [np.zeros((n, cfg.num_classes))]
        softmax = torch.nn.Softmax(1)

        def reference_route():
            stacked_probs = softmax(outputs).cpu().detach().numpy()
            s_points = batch.points[0].cpu().numpy()
            lengths = batch.lengths[0].cpu().numpy()
            in_inds = batch.input_inds.cpu().numpy()
            cloud_inds = batch.cloud_inds.cpu().numpy()
            torch.cuda.synchronize(dev)
            i0 = 0
            for b_i, length in enumerate(lengths):
                points, probs, inds = s_points[i0:i0 + length], stacked_probs[i0:i0 + length], in_inds[i0:i0 + length]
                c_i = cloud_inds[b_i]
                mask = np.sum(points ** 2, axis=1) < (ratio * cfg.in_radius) ** 2
                inds, probs = inds[mask], probs[mask]
                host_votes[c_i][inds] = smooth * host_votes[c_i][inds] + (1 - smooth) * probs
                i0 += length

        acc = tester.VoteAccumulator([n], cfg.num_classes, np.arange(cfg.num_classes), [], dev, smooth=smooth)
        t_ref = median_ms(reference_route, calls)
        t_dev = median_ms(lambda: acc.update(batch, outputs, radius_ratio=ratio, in_radius=cfg.in_radius), calls)

    for tag, t in (("(i)   forward, unfrozen", t_unfrozen), ("(ii)  forward, frozen", t_frozen),
                   ("(iii) vote, reference route (softmax -> host -> NumPy)", t_ref),
                   ("(iv)  vote, VoteAccumulator.update", t_dev)):
        lines.append("%-58s %8.3f  [%8.3f .. %8.3f]" % ((tag,) + t))
    lines.append("(ii) / (i) = %.3f    (iv) / (iii) = %.4f" % (t_frozen[0] / t_unfrozen[0], t_dev[0] / t_ref[0]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
