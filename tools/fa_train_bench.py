"""Development-only (GPU box): MVPNet3D's 2D -> 3D hand-off in training mode with and without
fuse_training(net, aggregation=True) (row kernels: csrc/pn2_rows.hip).

Workload: the default FeatureAggregation(64, (64, 64, 64)), sum over k, with relation features; nv = 3 views of h x w =
120 x 160, np = 8 192 points per chunk, k = 3 pixels per point, batches of 1, 8 and 32 chunks; the encoder's map
(B*nv, 64, 120, 160) NCHW and channels-last, requiring a gradient (a trained encoder) and not (a frozen one).
  hand-off        forward + backward from the map to the aggregated (B, 64, np) features alone: unfused = MVPNet3D.forward's
                  own steps (transposed copy of the map, two group_points, cat, Conv2d + BatchNorm2d + ReLU, torch.sum),
                  fused = FeatureAggregation.forward_rows (ops.pn2_fa_rows, ops.linear + ops.bn_lrelu per layer,
                  ops.pn2_rows_sum)
  whole network   forward + backward of out.square().mean() of an MVPNet3D whose encoder returns the stored map and whose
                  3D network is the default PN2SSG(64, 20), point search included: nothing fused; the 3D network fused
                  (fuse_training(net), the hand-off as the parent of this change runs it); the 3D network and the
                  aggregation fused (fuse_training(net, aggregation=True))
The paths of a row are timed in turn inside one loop in one process, so that they see the same clocks: HIP events around
each call after a device synchronisation, median [min .. max] milliseconds of 20 calls after 5 warm-up calls of each
path. torch.cuda.max_memory_allocated is recorded per path over its timed calls (MiB, the weights and inputs included).
Default mode (atomic backwards); nothing is asserted. The measurement runs in ONE child process under a time limit (the
parent never touches the GPU).
usage: python tools/fa_train_bench.py [out.txt] [calls] [batches, e.g. 1,8,32]     (default profiles/fa_train_bench.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 900
NV, H, W, NP, K, C = 3, 120, 160, 8192, 3, 64


def child(out_path, calls, batches):
    import torch
    from pn2_train_bench import WARMUP, alternating
    sys.path.insert(0, ROOT)
    import mvkpconv
    ops = mvkpconv.sub("ops")
    modules = mvkpconv.sub("dropin.mvpnet.models.pn2.modules")
    m3 = mvkpconv.sub("dropin.mvpnet.models.mvpnet_3d")
    PN2SSG = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    dev = torch.device("cuda:0")
    rows = []

    class MapEncoder(torch.nn.Module):
        def __init__(self, fmap):
            super().__init__()
            self.map = torch.nn.Parameter(fmap)

        def forward(self, data):
            return {"feature": self.map}

    def report(label, res):
        base = res["unfused"][0][0]
        cells = ["%s %9.3f [%9.3f .. %9.3f] %9.0f MiB" % ((k,) + t + (m,)) for k, (t, m) in res.items()]
        ratios = ["unfused / %s %5.2f" % (k, base / t[0]) for k, (t, m) in res.items() if k != "unfused"]
        rows.append("%-44s %s   %s" % (label, "   ".join(cells), "   ".join(ratios)))
        print(rows[-1], flush=True)

    for B in batches:
        for layout in ("nchw", "channels_last"):
            for needs_grad in (True, False):
                torch.manual_seed(B)
                fmap = torch.randn(B * NV, C, H, W, device=dev)
                if layout == "channels_last":
                    fmap = fmap.contiguous(memory_format=torch.channels_last)
                fmap.requires_grad_(needs_grad)
                image_xyz = torch.rand(B, NV, H, W, 3, device=dev)
                index = torch.randint(0, NV * H * W, (B, NP, K), device=dev)
                points = torch.rand(B, 3, NP, device=dev)
                tag = "B=%-2d %-13s map grad %-3s" % (B, layout, "yes" if needs_grad else "no")

                fa = m3.FeatureAggregation(C).to(dev).train()
                go = torch.randn(B, fa.out_channels, NP, device=dev)

                def handoff(fused):
                    fa.zero_grad(set_to_none=True)
                    fmap.grad = None
                    if fused:
                        out = fa.forward_rows(fmap, image_xyz, index, points)
                    else:
                        f = fmap.reshape(B, NV, -1, H, W).transpose(1, 2).contiguous().reshape(B, -1, NV * H * W)
                        f = ops.group_points(f, index)
                        with torch.no_grad():
                            xyz = ops.group_points(image_xyz.permute(0, 4, 1, 2, 3).reshape(B, 3, NV * H * W), index)
                        out = fa(xyz, points, f)
                    out.backward(go)

                report(tag + " hand-off", alternating({"unfused": lambda: handoff(False), "fused": lambda: handoff(True)},
                                                      calls))
                del fa, go

                net = m3.MVPNet3D(MapEncoder(fmap.detach()), None, PN2SSG(C, 20), in_channels=C).to(dev).train()
                net.net_2d.map.requires_grad_(needs_grad)
                batch = {"images": torch.zeros(B, NV, 3, H, W, device=dev), "image_xyz": image_xyz, "knn_indices": index,
                         "points": points}

                def step(fuse_3d, aggregation):
                    modules.unfuse_training(net)
                    if fuse_3d:
                        modules.fuse_training(net, aggregation=aggregation)
                    net.zero_grad(set_to_none=True)
                    net(batch)["seg_logit"].square().mean().backward()

                report(tag + " whole network",
                       alternating({"unfused": lambda: step(False, False), "fused 3D": lambda: step(True, False),
                                    "fused 3D + aggregation": lambda: step(True, True)}, calls))
                del net, batch, fmap, image_xyz, index, points
                torch.cuda.empty_cache()

    head = ("fa_train_bench: %s, FeatureAggregation(64, (64, 64, 64)) on nv=%d views of %dx%d, np=%d, k=%d; whole network = "
            "MVPNet3D with a stored map and PN2SSG(64, 20); training mode, forward + backward; median [min .. max] ms of %d "
            "calls after %d warm-ups, the paths of a row in turn, HIP events; peak MiB of torch.cuda.max_memory_allocated"
            % (torch.cuda.get_device_name(0), NV, H, W, NP, K, calls, WARMUP))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join([head] + rows) + "\n")


def main():
    argv = sys.argv
    if len(argv) > 1 and argv[1] == "--child":
        return child(argv[2], int(argv[3]), [int(v) for v in argv[4].split(",")])
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "fa_train_bench.txt")
    calls = argv[2] if len(argv) > 2 else "20"
    batches = argv[3] if len(argv) > 3 else "1,8,32"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out_path, calls, batches],
                       timeout=TIME_LIMIT_S)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
