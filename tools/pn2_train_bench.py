"""Development-only (GPU box): a PointNet++ training step with and without fuse_training (the row kernels
are csrc/pn2_rows.hip).

Workload: the default PN2SSG with 64 input channels and 20 classes on 8 192 points per chunk, training mode, batches of
1, 8 and 32 chunks.
  whole network   forward + backward of the loss-free step out.square().mean(), point search included
  sa0 .. sa3      one SetAbstraction alone on its real inputs (the previous level's output of the same network), forward +
                  backward; the point search is excluded: farthest point sampling and the ball query return the indices
                  of an earlier call
Per row the unfused path (unfuse_training: Conv2d + BatchNorm2d + torch.max on (B,C,M,K) tensors) and the fused path
(fuse_training: ops.pn2_sa_rows, ops.linear + ops.bn_lrelu per layer, ops.pn2_rows_max) are timed in turn inside one loop
in one process, so that they see the same clocks: HIP events around each call after a device synchronisation, median
[min .. max] milliseconds of 20 calls after 5 warm-up calls of each path. torch.cuda.max_memory_allocated is recorded per
path over its timed calls (MiB, the weights and inputs included). Default mode (atomic backwards); nothing is asserted.
The measurement runs in ONE child process under a time limit (the parent never touches the GPU).
usage: python tools/pn2_train_bench.py [out.txt] [calls] [batches, e.g. 1,8,32]     (default profiles/pn2_train_bench.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 540
WARMUP = 5


def alternating(fns, calls):
    """{label: ((median, min, max) ms, peak MiB)} with the callables timed in turn inside one loop."""
    import numpy as np
    import torch
    for _ in range(WARMUP):
        for fn in fns.values():
            fn()
    times, peak = {k: [] for k in fns}, {k: 0 for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            times[k].append(e0.elapsed_time(e1))
            peak[k] = max(peak[k], torch.cuda.max_memory_allocated())
    return {k: ((float(np.median(v)), float(np.min(v)), float(np.max(v))), peak[k] / 2.0 ** 20) for k, v in times.items()}


def child(out_path, calls, batches):
    import torch
    sys.path.insert(0, ROOT)
    import mvkpconv
    modules = mvkpconv.sub("dropin.mvpnet.models.pn2.modules")
    PN2SSG = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg").PN2SSG
    dev = torch.device("cuda:0")
    rows = []

    def report(label, res):
        (tu, mu), (tf, mf) = res["unfused"], res["fused"]
        rows.append("%-28s unfused %9.3f [%9.3f .. %9.3f] %9.0f MiB   fused %9.3f [%9.3f .. %9.3f] %9.0f MiB   "
                    "unfused / fused %5.2f" % ((label,) + tu + (mu,) + tf + (mf, tu[0] / tf[0])))
        print(rows[-1], flush=True)

    for B in batches:
        torch.manual_seed(B)
        net = PN2SSG(64, 20).to(dev).train()
        batch = {"points": torch.rand(B, 3, 8192, device=dev), "feature": torch.randn(B, 64, 8192, device=dev)}
        params = [p for p in net.parameters()]

        def step(fused):
            (modules.fuse_training if fused else modules.unfuse_training)(net)
            net.zero_grad(set_to_none=True)
            net(batch)["seg_logit"].square().mean().backward()

        report("B=%-2d whole network" % B, alternating({"unfused": lambda: step(False), "fused": lambda: step(True)}, calls))

        # the real inputs of every level and the indices of its point search, from one unfused forward
        modules.unfuse_training(net)
        real_fps, real_bq = modules.farthest_point_sample, modules.ball_query
        try:
            xyz, feature = batch["points"], batch["feature"]
            for lv, sa in enumerate(net.sa_modules):
                found = {}

                def once(key, fn, found=found):
                    def cached(*a, **k):
                        if key not in found:
                            found[key] = fn(*a, **k)
                        return found[key]
                    return cached

                modules.farthest_point_sample, modules.ball_query = once("fps", real_fps), once("bq", real_bq)
                with torch.no_grad():
                    nxt = sa(xyz, feature)                       # fills `found`; later calls return the same tensors
                x_in = xyz.detach()
                f_in = feature.detach().clone().requires_grad_(True)
                go = torch.randn_like(nxt[1])

                def sa_step(fused, sa=sa, x_in=x_in, f_in=f_in, go=go):
                    sa._fused_training = fused
                    sa.zero_grad(set_to_none=True)
                    f_in.grad = None
                    sa(x_in, f_in)[1].backward(go)

                label = "B=%-2d sa%d %s" % (B, lv, "x".join(str(v) for v in (sa.in_channels,) + tuple(
                    layer.conv.out_channels for layer in sa.mlp)))
                report(label, alternating({"unfused": lambda: sa_step(False), "fused": lambda: sa_step(True)}, calls))
                xyz, feature = nxt[0].detach(), nxt[1].detach()
        finally:
            modules.farthest_point_sample, modules.ball_query = real_fps, real_bq
        del net, batch, params
        torch.cuda.empty_cache()

    head = ("pn2_train_bench: %s, PN2SSG(64, 20) on 8192 points, training mode, forward + backward; median [min .. max] ms "
            "of %d calls after %d warm-ups, both paths in turn, HIP events; peak MiB of torch.cuda.max_memory_allocated"
            % (torch.cuda.get_device_name(0), calls, WARMUP))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join([head] + rows) + "\n")


def main():
    argv = sys.argv
    if len(argv) > 1 and argv[1] == "--child":
        return child(argv[2], int(argv[3]), [int(v) for v in argv[4].split(",")])
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "pn2_train_bench.txt")
    calls = argv[2] if len(argv) > 2 else "20"
    batches = argv[3] if len(argv) > 3 else "1,8,32"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out_path, calls, batches],
                       timeout=TIME_LIMIT_S)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
