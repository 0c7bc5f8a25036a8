"""Development-only (GPU box): the MVPNet whole-scene test with several chunks per forward on the synthetic
room of tools/chunk_bench.py (200 000 points in 8 x 6 x 3 m, part of the floor plan thinned; chunks of 1.5 m, stride 0.5,
margin 0.2, threshold 1000; 20 classes).

The network is the default PN2SSG (64 input channels, 20 classes) after freeze_inference. Its input features come
straight from a per-point table of the scene (a gather by the chunk's point indices stands for the 2D encoder and the
feature aggregation), so what is timed is the loop itself: padding and collation of the chunks, the PointNet++ forward
and the votes.

predict_whole_scene_grouped(chunks_per_forward=G) for G in {1, 4, 16, 32}; G = 1 is predict_whole_scene, the baseline.
The settings alternate scene by scene in one process: 5 warm-up rounds, then `scenes` timed rounds (default 20), each scene
between two HIP events after a device synchronisation. Reported: median [min .. max] milliseconds per scene, the number
of forwards, and the padded-column overhead (sum over the groups of group size x largest chunk, over the sum of the chunk
sizes). The mean logits and predictions of every G are compared with those of G = 1 on the same scene.

Writes profiles/pn2_ragged_bench.txt (or the path given).  usage: python tools/pn2_ragged_bench.py [out.txt] [scenes]"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvkpconv
import chunk_ref

chunk_util = mvkpconv.sub("dropin.mvpnet.utils.chunk_util")
grouped = mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")
pn2ssg = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg")
dev = torch.device("cuda:0")
C, C_IN, MIN_NB_PTS = 20, 64, 2048
GROUPS = (1, 4, 16, 32)
ARGS = dict(chunk_size=(1.5, 1.5), stride=0.5, thresh=1000, margin=(0.2, 0.2))


class DirectFeatures(torch.nn.Module):
    """The 3D network fed from a per-point feature table of the scene: 'knn_indices' (B, N, 1) holds each point's row."""

    def __init__(self, net_3d, table):
        super().__init__()
        self.net_3d, self.table = net_3d, table                         # table (C_IN, num_points)

    def forward(self, batch):
        rows = batch["knn_indices"][..., 0]                             # (B, N); padded rows are 0, a valid row
        batch_3d = {"points": batch["points"], "feature": self.table[:, rows].transpose(0, 1).contiguous()}
        if "lengths" in batch:
            batch_3d["lengths"] = batch["lengths"]
        return self.net_3d(batch_3d)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pn2_ragged_bench.txt")
    scenes = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = 5
    points = chunk_ref.random_scene(0, 310000, ext=(8.0, 6.0, 3.0))[:200000]
    n = len(points)
    pts = torch.from_numpy(points).to(dev)
    indices, _ = chunk_util.scene2chunks_legacy(pts, return_bbox=True, **ARGS)
    sizes = [max(len(i), MIN_NB_PTS) for i in indices]
    inputs = [{"points": pts[ind].t().contiguous(), "chunk_ind": ind, "knn_indices": ind[:, None].contiguous()}
              for ind in indices]

    torch.manual_seed(0)
    net_3d = pn2ssg.PN2SSG(C_IN, C).to(dev).eval()
    table = torch.randn((C_IN, n), device=dev)
    model = pn2ssg.freeze_inference(DirectFeatures(net_3d, table)).eval()
    assert all(m._frozen is not None for m in list(net_3d.sa_modules) + list(net_3d.fp_modules) + [net_3d])

    def scene(g):
        np.random.seed(0)                                               # the pad draws of sparse chunks
        return grouped.predict_whole_scene_grouped(model, pts, inputs, min_nb_pts=MIN_NB_PTS, chunks_per_forward=g)

    times = {g: [] for g in GROUPS}
    for it in range(warmup + scenes):
        for g in GROUPS:
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            scene(g)
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                times[g].append(e0.elapsed_time(e1))

    pred1, mean1 = scene(1)
    top = torch.sort(mean1, dim=1).values
    margin = top[:, -1] - top[:, -2]
    lines = ["pn2_ragged_bench: %d points, %d chunks of %d .. %d points (sum %d, %d below min_nb_pts = %d and padded to it), "
             "PN2SSG(%d, %d) frozen; predict_whole_scene_grouped, median [min .. max] ms per scene over %d scenes after %d "
             "warm-ups, settings alternating" % (n, len(indices), min(len(i) for i in indices), max(len(i) for i in indices),
                                       sum(len(i) for i in indices), sum(len(i) < MIN_NB_PTS for i in indices), MIN_NB_PTS,
                                       C_IN, C, scenes, warmup)]
    for g in GROUPS:
        groups = [sizes[i:i + g] for i in range(0, len(sizes), g)]
        overhead = sum(len(gr) * max(gr) for gr in groups) / float(sum(sizes))
        pred, mean = scene(g)
        diff = (mean - mean1).abs().max(dim=1).values
        flipped = pred != pred1
        t = times[g]
        lines.append("G = %2d   %9.3f [%9.3f .. %9.3f] ms   %3d forwards   G=1 / G %5.2f   padded columns / chunk columns %6.4f   "
                     "largest |mean logit - G=1| %.3e   predictions that differ %d (%d of them where the G=1 margin exceeds the "
                     "point's difference)"
                     % (g, np.median(t), np.min(t), np.max(t), len(groups), np.median(times[1]) / np.median(t), overhead,
                        float(diff.max()), int(flipped.sum()), int((flipped & (margin > diff)).sum())))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
