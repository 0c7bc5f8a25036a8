"""Development-only (GPU box): the 2D -> 3D hand-off of a frozen MVPNet3D as one fused launch (DESIGN 7l;
freeze_inference(net, aggregation=True), ops.pn2_fa_mlp, pn2_fa_k of csrc/pn2_mlp.hip) against the unfused path of the
same commit, in the same process.

1. The stage alone, from the encoder's output to feature_2d3d: the default FeatureAggregation(64) (68 -> 64 -> 64 -> 64,
   sum, relation features), k = 3, nv = 3 views of 120 x 160 pixels, BatchNorm statistics away from their initial values.
   Unfused: MVPNet3D.forward's own lines (transposed copy of the map, permuted copy of image_xyz, two group_points,
   FeatureAggregation.forward in eval mode). Fused: FeatureAggregation.from_encoder_map. Shapes: B = 1 x 8 192 points, and
   B = 32 chunks padded to the largest (sizes drawn from 3 698 .. 23 201, the range of the synthetic room's chunks; the
   fused call gets `lengths`, the unfused path computes the padded columns too, as it does inside the grouped loop).
   Each shape with the map contiguous (NCHW) and channels-last. The pixel indices are random, so a point's three pixels
   are not neighbours in the image as a real kNN's would be; both paths gather the same indices. The peak of
   torch.cuda.max_memory_allocated over one call, above what is allocated before it, is recorded for B = 32.
2. predict_whole_scene_grouped on the synthetic room of tools/pn2_ragged_bench.py (200 000 points, chunks of 1.5 m) at
   G in {1, 32} with an MVPNet3D whose 3D network is the default PN2SSG (64 input channels, 20 classes), frozen, and
   whose 2D ENCODER IS A CHEAP STAND-IN: one 1 x 1 convolution 3 -> 64 on nv = 3 random images of 120 x 160 per chunk,
   with random image_xyz inside the chunk's box and random pixel indices. A real encoder would add the same time to both
   columns; what is compared is the loop with the aggregation unfused (freeze_inference(net)) and fused
   (freeze_inference(net, aggregation=True)).

Times: median [min .. max] milliseconds between two HIP events after a device synchronisation, 20 calls after 5 warm-ups,
unfused and fused alternating. Writes profiles/pn2_fa_bench.txt (or the path given).
usage: python tools/pn2_fa_bench.py [out.txt] [calls]"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvkpconv
import chunk_ref

ops = mvkpconv.sub("ops")
m3 = mvkpconv.sub("dropin.mvpnet.models.mvpnet_3d")
pn2ssg = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg")
chunk_util = mvkpconv.sub("dropin.mvpnet.utils.chunk_util")
grouped = mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")
dev = torch.device("cuda:0")
C2D, NV, H, W, K, CLASSES, MIN_NB_PTS = 64, 3, 120, 160, 3, 20, 2048
ARGS = dict(chunk_size=(1.5, 1.5), stride=0.5, thresh=1000, margin=(0.2, 0.2))


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


def peak_mib(fn):
    """Peak of the caching allocator's allocated bytes during one call, above what was allocated before it."""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2.0 ** 20


def perturb_batchnorm(net, rng):
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.from_numpy(1 + 0.1 * rng.standard_normal(m.weight.shape)).float())
                m.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_mean.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_var.copy_(torch.from_numpy(1 + 0.1 * np.abs(rng.standard_normal(m.bias.shape))).float())


def unfused_stage(fa, fmap, image_xyz, knn, points):
    """MVPNet3D.forward between the encoder and the 3D network, as it stands."""
    b, nv, h, w, _ = image_xyz.shape
    f = fmap.reshape(b, nv, -1, h, w).transpose(1, 2).contiguous().reshape(b, -1, nv * h * w)
    f = ops.group_points(f, knn)
    xyz = ops.group_points(image_xyz.permute(0, 4, 1, 2, 3).reshape(b, 3, nv * h * w), knn)
    return fa(xyz, points, f)


class StandIn2D(torch.nn.Module):
    """Stands for the 2D encoder: {'image': (n,3,h,w)} -> {'feature': (n,c,h,w)}, one 1 x 1 convolution."""

    def __init__(self, c):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, c, 1)

    def forward(self, data):
        return {"feature": self.conv(data["image"])}


def stage_rows(calls, lines):
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    fa = m3.FeatureAggregation(C2D).to(dev).eval()
    perturb_batchnorm(fa, rng)
    frozen = pn2ssg.freeze_inference(copy.deepcopy(fa), aggregation=True)
    snap = frozen._frozen
    assert snap is not None and snap[1] == (C2D + 4, 64, 64, 64)
    fmt = "%-44s unfused %9.3f [%9.3f .. %9.3f]   fused %8.3f [%8.3f .. %8.3f]   fused / unfused %6.3f"
    shapes = [("B =  1 x 8192 points", 1, [8192]), ("B = 32 padded chunks", 32, sorted(rng.integers(3698, 23202, size=32).tolist()))]
    for label, b, sizes in shapes:
        n = max(sizes)
        lengths = torch.tensor(sizes, dtype=torch.int64, device=dev) if b > 1 else None
        image_xyz = torch.rand(b, NV, H, W, 3, device=dev)
        points = torch.rand(b, 3, n, device=dev)
        knn = torch.randint(0, NV * H * W, (b, n, K), device=dev)
        for layout in ("NCHW", "channels-last"):
            fmap = torch.randn(b * NV, C2D, H, W, device=dev)
            if layout == "channels-last":
                fmap = fmap.contiguous(memory_format=torch.channels_last)
            un = lambda: unfused_stage(fa, fmap, image_xyz, knn, points)
            fu = lambda: frozen.from_encoder_map(snap, fmap, image_xyz, knn, points, lengths=lengths)
            a, c = un(), fu()
            valid = torch.arange(n, device=dev)[None, :] < (lengths[:, None] if b > 1 else n)
            rel = float(((a - c) * valid[:, None]).norm() / (a * valid[:, None]).norm())
            tu, tf = pair_ms(un, fu, calls)
            del a, c
            name = "%s, N = %d, map %s" % (label, n, layout)
            lines.append(fmt % ((name,) + tu + tf + (tf[0] / tu[0],)))
            lines.append("    L2-relative difference on the valid columns %.2e; fused max %s unfused min" %
                         (rel, "<" if tf[2] < tu[1] else ">="))
            if b > 1:
                pu, pf = peak_mib(un), peak_mib(fu)
                lines.append("    peak memory above the inputs: unfused %.1f MiB, fused %.1f MiB (difference %.1f MiB)" % (pu, pf, pu - pf))
            del fmap
        del image_xyz, points, knn
        torch.cuda.empty_cache()


def scene_rows(calls, lines):
    points = chunk_ref.random_scene(0, 310000, ext=(8.0, 6.0, 3.0))[:200000]
    pts = torch.from_numpy(points).to(dev)
    indices, _ = chunk_util.scene2chunks_legacy(pts, return_bbox=True, **ARGS)
    gen = torch.Generator(device=dev)
    gen.manual_seed(1)
    inputs = []
    for ind in indices:
        p = pts[ind]
        lo, hi = p.min(0).values, p.max(0).values
        inputs.append({"points": p.t().contiguous(), "chunk_ind": ind,
                       "images": torch.rand(NV, 3, H, W, device=dev, generator=gen),
                       "image_xyz": lo + (hi - lo) * torch.rand(NV, H, W, 3, device=dev, generator=gen),
                       "knn_indices": torch.randint(0, NV * H * W, (len(ind), K), device=dev, generator=gen)})
    torch.manual_seed(0)
    net = m3.MVPNet3D(StandIn2D(C2D), None, pn2ssg.PN2SSG(64, CLASSES), in_channels=C2D).to(dev).eval()
    perturb_batchnorm(net, np.random.default_rng(0))
    base = pn2ssg.freeze_inference(copy.deepcopy(net))
    fused = pn2ssg.freeze_inference(copy.deepcopy(net), aggregation=True)
    assert base.feat_aggreg._frozen is None and fused.feat_aggreg._frozen is not None and base.net_3d._frozen is not None

    def scene(model, g):
        np.random.seed(0)
        return grouped.predict_whole_scene_grouped(model, pts, inputs, min_nb_pts=MIN_NB_PTS, chunks_per_forward=g)

    lines.append("whole scene: %d points, %d chunks of %d .. %d points, nv = %d stand-in images of %d x %d per chunk (one 1 x 1 "
                 "convolution 3 -> %d as the 2D encoder), default PN2SSG(64, %d) frozen in both columns"
                 % (len(points), len(indices), min(len(i) for i in indices), max(len(i) for i in indices), NV, H, W, C2D, CLASSES))
    fmt = "%-44s unfused %9.3f [%9.3f .. %9.3f]   fused %8.3f [%8.3f .. %8.3f]   fused / unfused %6.3f"
    for g in (1, 32):
        (pa, ma), (pb, mb) = scene(base, g), scene(fused, g)
        diff = float((ma - mb).abs().max())
        tu, tf = pair_ms(lambda: scene(base, g), lambda: scene(fused, g), calls)
        lines.append(fmt % (("predict_whole_scene_grouped, G = %d" % g,) + tu + tf + (tf[0] / tu[0],)))
        lines.append("    largest |mean logit difference| %.3e, predictions that differ %d of %d; fused max %s unfused min"
                     % (diff, int((pa != pb).sum()), len(points), "<" if tf[2] < tu[1] else ">="))
        if g == 32:
            pu, pf = peak_mib(lambda: scene(base, g)), peak_mib(lambda: scene(fused, g))
            lines.append("    peak memory above the scene's inputs: unfused %.1f MiB, fused %.1f MiB (difference %.1f MiB)" % (pu, pf, pu - pf))


class Lines(list):
    """The report's lines, shown as they come."""

    def append(self, line):
        print(line, flush=True)
        list.append(self, line)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pn2_fa_bench.txt")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    lines = Lines()
    lines.append("pn2_fa_bench: FeatureAggregation(%d) 68 -> 64 -> 64 -> 64, sum, k = %d, nv = %d views of %d x %d; eval, no_grad; "
             "median [min .. max] ms by HIP events, %d alternating calls after 5 warm-ups" % (C2D, K, NV, H, W, calls))
    with torch.no_grad():
        stage_rows(calls, lines)
        scene_rows(calls, lines)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
