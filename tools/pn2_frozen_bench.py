"""Development-only (GPU box): the frozen inference forward of the MVPNet baseline's PointNet++ (freeze_inference,
dropin/mvpnet/models/pn2; csrc/pn2_mlp.hip) against the unfrozen eval forward, in the same process.

Network: the default PN2SSG (four SetAbstraction levels 2048 / 512 / 128 / 32 centroids, K = 32; four FeaturePropagation
levels; mlp_seg + seg_logit), in_channels 64, 20 classes, BatchNorm statistics away from their initial values. Input:
B = 1, one synthetic chunk of 8192 and one of 16 384 points on a floor and two walls of a 1.5 x 1.5 x 3 m box, eval mode
under torch.no_grad().

Rows: the whole forward, then per module the part that freezing replaces, on that module's real inputs with the point
search (farthest point sampling, ball query, 3-NN and weights) done beforehand and excluded: "group, concatenate,
SharedMLP, max" against one pn2_sa_mlp_max launch, "interpolate, concatenate, SharedMLP" against one pn2_fp_mlp launch.
Times: median [min .. max] milliseconds between two HIP events after a device synchronisation, 20 calls after 5
warm-ups, the unfrozen and the frozen call alternating. The frozen forward counts as faster when its max is below the
unfrozen min.
Writes profiles/pn2_frozen_bench.txt (or the path given).  usage: python tools/pn2_frozen_bench.py [out.txt] [calls]"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvkpconv

ops = mvkpconv.sub("ops")
modules = mvkpconv.sub("dropin.mvpnet.models.pn2.modules")
PN2SSG = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
dev = torch.device("cuda:0")


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


def chunk_points(n, seed):
    """n points on the floor and two walls of a 1.5 x 1.5 x 3 m box, (1, 3, n) float32."""
    rng = np.random.default_rng(seed)
    u, v = rng.random(n), rng.random(n)
    face = rng.choice(3, size=n, p=[0.2, 0.4, 0.4])
    x = np.where(face == 2, 0.0, 1.5 * u)
    y = np.where(face == 1, 0.0, np.where(face == 0, 1.5 * v, 1.5 * u))
    z = np.where(face == 0, 0.0, 3.0 * v)
    pts = np.stack([x, y, z]) + 0.01 * rng.standard_normal((3, n))
    return torch.from_numpy(pts[None].astype(np.float32)).to(dev)


def make_net():
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    net = PN2SSG(64, 20).to(dev).eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.from_numpy(1 + 0.1 * rng.standard_normal(m.weight.shape)).float())
                m.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_mean.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_var.copy_(torch.from_numpy(1 + 0.1 * np.abs(rng.standard_normal(m.bias.shape))).float())
    return net


def level_stages(net, frozen, batch):
    """[(label, unfrozen callable, frozen callable)] per module, on the inputs one unfrozen forward gives it."""
    stages = []
    xyz, feature = batch["points"], batch["feature"]
    xyzs, feats = [xyz], [None]
    for lv, (sa, fsa) in enumerate(zip(net.sa_modules, frozen.sa_modules)):
        new_xyz = modules.batch_index_select(xyz, modules.farthest_point_sample(xyz, sa.num_centroids), dim=2)
        index = modules.ball_query(new_xyz, xyz, sa.radius, sa.max_neighbors)

        def unfused(sa=sa, xyz=xyz, feature=feature, new_xyz=new_xyz, index=index):
            x = torch.cat([modules.group_points(feature, index), modules.group_points(xyz, index) - new_xyz.unsqueeze(-1)], dim=1)
            return torch.max(sa.mlp(x), dim=3)[0]

        def fused(fsa=fsa, xyz=xyz, feature=feature, new_xyz=new_xyz, index=index):
            return ops.pn2_sa_mlp_max(xyz, feature, new_xyz, index, *fsa._frozen)

        stages.append(("sa%d  %5d x %2d rows, widths %s" % (lv, new_xyz.shape[2], index.shape[2], list(fsa._frozen[1])), unfused, fused))
        xyz, feature = new_xyz.contiguous(), unfused()
        xyzs.append(xyz)
        feats.append(feature)
    up = feats[-1]
    for lv, (fp, ffp) in enumerate(zip(net.fp_modules, frozen.fp_modules)):
        dense_xyz, sparse_xyz, dense = xyzs[-2 - lv], xyzs[-1 - lv], feats[-2 - lv]
        index, weight = fp.interpolator.weights(dense_xyz, sparse_xyz)

        def unfused(fp=fp, up=up, index=index, weight=weight, dense=dense):
            x = modules.feature_interpolate(up, index, weight)
            return fp.mlp(x if dense is None else torch.cat([x, dense], dim=1))

        def fused(ffp=ffp, up=up, index=index, weight=weight, dense=dense):
            return ops.pn2_fp_mlp(up, index, weight, dense, *ffp._frozen)

        stages.append(("fp%d  %5d rows,      widths %s" % (lv, dense_xyz.shape[2], list(ffp._frozen[1])), unfused, fused))
        up = unfused()
    stages.append(("head %5d rows,      widths %s" % (up.shape[2], list(frozen._frozen[1])),
                   lambda up=up: net.seg_logit(net.mlp_seg(up)),
                   lambda up=up: ops.pn2_fp_mlp(None, None, None, up, *frozen._frozen, relu_last=False)))
    return stages


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "pn2_frozen_bench.txt")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    net = make_net()
    frozen = modules.freeze_inference(copy.deepcopy(net))
    assert all(m._frozen is not None for m in frozen.modules() if isinstance(m, modules.Freezable))
    fmt = "%-58s unfrozen %8.3f [%8.3f .. %8.3f]   frozen %8.3f [%8.3f .. %8.3f]   frozen / unfrozen %5.2f"
    lines = ["pn2_frozen_bench: default PN2SSG, in_channels 64, 20 classes, B = 1, eval, no_grad; median [min .. max] ms by "
             "HIP events, %d alternating calls after 5 warm-ups" % calls]
    with torch.no_grad():
        for n in (8192, 16384):
            batch = {"points": chunk_points(n, n), "feature": torch.randn(1, 64, n, device=dev)}
            a, b = net(batch)["seg_logit"], frozen(batch)["seg_logit"]
            rel = float((a - b).norm() / a.norm())
            lines.append("chunk of %d points (frozen vs unfrozen logits: L2-relative difference %.2e)" % (n, rel))
            tu, tf = pair_ms(lambda: net(batch), lambda: frozen(batch), calls)
            lines.append(fmt % (("whole forward",) + tu + tf + (tf[0] / tu[0],)))
            lines.append("    frozen max %s unfrozen min: %s" % (("<", "faster beyond the spread") if tf[2] < tu[1]
                                                                  else (">=", "NOT faster beyond the spread")))
            for label, unfused, fused in level_stages(net, frozen, batch):
                tu, tf = pair_ms(unfused, fused, calls)
                lines.append(fmt % (("  " + label,) + tu + tf + (tf[0] / tu[0],)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
