"""Development-only (GPU box): the point ops of the MVPNet baseline (csrc/pn2.hip) against what a user could write in
plain torch on the same GPU, at the shapes of the reference's own profile cases and of PN2SSG's first level:

  fps            32 x 8192 -> 2048        torch: a Python loop of torch ops (one round = distance, minimum, argmax)
  ball query     32 x (512 of 1024), K=64 and 8 x (2048 of 8192), r=0.1, K=32
                                          torch: cdist, mask, sort of the masked key indices, first K, padding
  3-NN           8 x 8192 queries x 2048 keys
                                          torch: cdist + topk
  interpolation  32 x 64 x 2048 -> 8192, forward and backward
                                          torch: gather, weighted sum, autograd

  ordered backwards (csrc/pn2_ordered.hip), library calls into preallocated outputs, the forms of one op timed in turn
  inside one loop (atomic, ordered, atomic, ordered, ...), so that they see the same clocks:
    interpolation bwd  32 x 64 x 2048 -> 8192 (the row above)
    group_points bwd   8 x 64 channels, 8192 keys, index 2048 x 32 from a ball query (a first set abstraction)
  per op: the atomic kernel alone, the zero fill it needs + the atomic kernel, the ordered kernel alone, the CSR build
  alone, and the CSR build + the ordered kernel (what a backward costs when nobody built the CSR before).

Median milliseconds over eager calls, each bracketed by HIP events after a device synchronisation. The torch columns do
not reproduce the reference's tie order or its rounding; they are the cost of the obvious formulation, not a referee.
The measurement runs in ONE child process under a time limit (the parent never touches the GPU).
usage: python tools/pn2_bench.py [out.txt] [calls] [--ordered]     (default profiles/pn2_bench.txt, 20 calls;
       --ordered: only the ordered-backward rows, APPENDED to out.txt)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIME_LIMIT_S = 420


def median_ms(fn, calls, warmup=2):
    import numpy as np
    import torch
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


def alternating_ms(fns, calls, warmup=2):
    """{label: (median, min, max)} with the callables timed in turn inside one loop."""
    import numpy as np
    import torch
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    out = {k: [] for k in fns}
    for _ in range(calls):
        for k, fn in fns.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return {k: (float(np.median(v)), float(np.min(v)), float(np.max(v))) for k, v in out.items()}


def ordered_rows(ops, dev, calls, rows):
    """The two scattering backwards: atomic form against ordered form, library calls on preallocated buffers."""
    import torch
    lib, check, p, st = ops.lib(), ops.check, ops._p, ops._stream

    def section(label, atomic, ordered, index, n1, gi, added_bytes):
        csr = {}

        def build():
            csr["rs"], csr["en"] = ops.index_csr(index, n1)

        build()
        times = alternating_ms({
            "atomic kernel alone": atomic,
            "zero fill + atomic kernel": lambda: (gi.zero_(), atomic()),
            "ordered kernel alone": lambda: ordered(csr["rs"], csr["en"]),
            "CSR build alone": build,
            "CSR build + ordered kernel": lambda: (build(), ordered(csr["rs"], csr["en"])),
        }, calls)
        base = times["zero fill + atomic kernel"][0]
        for k, t in times.items():
            rows.append("%-46s %-28s %9.3f [%9.3f .. %9.3f]   (zero fill + atomic) / this %6.2f%s"
                        % ((label, k) + t + (base / t[0], "   %.3f TB/s of added bytes" % (added_bytes / t[0] * 1e-9)
                                             if k == "atomic kernel alone" else "")))
            print(rows[-1], flush=True)

    B, C, N1, N2 = 32, 64, 2048, 8192
    index = torch.randint(0, N1, (B, N2, 3), device=dev)
    weight = torch.rand(B, N2, 3, device=dev)
    weight = weight / weight.sum(2, keepdim=True)
    go = torch.randn(B, C, N2, device=dev)
    gi = torch.zeros(B, C, N1, device=dev)
    status = ops.pn2_index_status(dev)
    section("interpolation bwd 32 x 64 x 2048 -> 8192",
            lambda: check(lib.mvk_interpolate_bwd(p(go), p(index), p(weight), B, C, N1, N2, p(gi), p(status), st())),
            lambda rs, en: check(lib.mvk_interpolate_bwd_csr(p(go), p(weight), p(rs), p(en), B, C, N1, N2, p(gi), st())),
            index, N1, gi, 4.0 * B * C * N2 * 3)

    B, C, N1, N2, K = 8, 64, 8192, 2048, 32
    key = torch.rand(B, N1, 3, device=dev)
    gindex = ops.pn2_ball_query(key[:, :N2].contiguous(), key, 0.1, K)
    ggo = torch.randn(B, C, N2, K, device=dev)
    ggi = torch.zeros(B, C, N1, device=dev)
    section("group_points bwd 8 x 64 x 8192 <- 2048 x 32",
            lambda: check(lib.mvk_group_points_bwd(p(ggo), p(gindex), B, C, N1, N2, K, p(ggi), st())),
            lambda rs, en: check(lib.mvk_group_points_bwd_csr(p(ggo), p(rs), p(en), B, C, N1, N2, K, p(ggi), st())),
            gindex, N1, ggi, 4.0 * B * C * N2 * K)


def torch_fps(pts, m):
    import torch
    b = pts.shape[0]
    ar = torch.arange(b, device=pts.device)
    cur = torch.zeros(b, dtype=torch.int64, device=pts.device)
    run = torch.full(pts.shape[:2], float("inf"), device=pts.device, dtype=pts.dtype)
    out = [cur]
    for _ in range(1, m):
        d = ((pts - pts[ar, cur][:, None]) ** 2).sum(-1)
        run = torch.minimum(run, d)
        cur = run.argmax(1)
        out.append(cur)
    return torch.stack(out, 1)


def torch_ball_query(q, key, radius, k):
    import torch
    n2 = key.shape[1]
    inside = torch.cdist(q, key) ** 2 < radius * radius
    cand = torch.where(inside, torch.arange(n2, device=q.device), torch.full((), n2, device=q.device))
    first = cand.sort(dim=2)[0][..., :k]
    pad = first[..., :1].expand_as(first)
    idx = torch.where(first < n2, first, pad)
    return torch.where(idx < n2, idx, torch.full((), -1, device=q.device))


def torch_knn(q, key):
    import torch
    d, i = (torch.cdist(q, key) ** 2).topk(3, dim=2, largest=False, sorted=True)
    return i, d


def torch_interpolate(feature, index, weight):
    import torch
    b, c, n1 = feature.shape
    n2 = index.shape[1]
    g = torch.gather(feature.unsqueeze(2).expand(b, c, n2, n1), 3, index.unsqueeze(1).expand(b, c, n2, 3))
    return (g * weight.unsqueeze(1)).sum(-1)


def child(out_path, calls, ordered_only=False):
    import torch
    sys.path.insert(0, ROOT)
    import mvkpconv
    ops = mvkpconv.sub("ops")
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    rows = []
    if ordered_only:
        head = ("pn2_bench --ordered: %s, median [min .. max] ms of %d eager calls, the forms of one op in turn, HIP events"
                % (torch.cuda.get_device_name(0), calls))
        ordered_rows(ops, dev, calls, rows)
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "a") as f:
            f.write("\n".join([head] + rows) + "\n")
        return

    def row(label, hip, ref, n_ref_calls, extra=""):
        t_hip = median_ms(hip, calls)
        t_ref = median_ms(ref, n_ref_calls, warmup=1)
        rows.append("%-46s HIP %9.3f [%9.3f .. %9.3f]   torch %9.3f [%9.3f .. %9.3f]   torch / HIP %7.2f%s"
                    % ((label,) + t_hip + t_ref + (t_ref[0] / t_hip[0], extra)))
        print(rows[-1], flush=True)
        return t_hip

    pts = torch.rand(32, 8192, 3, device=dev)
    t = median_ms(lambda: ops.fps(pts, 2048), calls)
    t_ref = median_ms(lambda: torch_fps(pts, 2048), 2, warmup=1)
    rows.append("%-46s HIP %9.3f [%9.3f .. %9.3f]   torch %9.3f [%9.3f .. %9.3f]   torch / HIP %7.2f   %.3f us per round"
                % (("fps 32 x 8192 -> 2048 (f32)",) + t + t_ref + (t_ref[0] / t[0], 1e3 * t[0] / 2047)))
    print(rows[-1], flush=True)
    one = pts[:1].contiguous()
    t1 = median_ms(lambda: ops.fps(one, 2048), calls)
    rows.append("%-46s HIP %9.3f [%9.3f .. %9.3f]   %.3f us per round (one workgroup alone)"
                % (("fps  1 x 8192 -> 2048 (f32)",) + t1 + (1e3 * t1[0] / 2047,)))
    print(rows[-1], flush=True)

    key = torch.randn(32, 1024, 3, device=dev)
    q = key[:, :512].contiguous()
    row("ball query 32 x (512 of 1024), r=0.1, K=64", lambda: ops.pn2_ball_query(q, key, 0.1, 64),
        lambda: torch_ball_query(q, key, 0.1, 64), 5)
    key = torch.rand(8, 8192, 3, device=dev)
    q = key[:, :2048].contiguous()
    row("ball query 8 x (2048 of 8192), r=0.1, K=32", lambda: ops.pn2_ball_query(q, key, 0.1, 32),
        lambda: torch_ball_query(q, key, 0.1, 32), 5)

    q, key = torch.randn(8, 8192, 3, device=dev), torch.randn(8, 2048, 3, device=dev)
    row("3-NN 8 x 8192 queries x 2048 keys", lambda: ops.knn_distance(q, key, 3), lambda: torch_knn(q, key), 5)

    feature = torch.randn(32, 64, 2048, device=dev, requires_grad=True)
    index = torch.randint(0, 2048, (32, 8192, 3), device=dev)
    weight = torch.rand(32, 8192, 3, device=dev)
    weight = weight / weight.sum(2, keepdim=True)
    row("interpolation fwd 32 x 64 x 2048 -> 8192", lambda: ops.feature_interpolate(feature, index, weight),
        lambda: torch_interpolate(feature, index, weight), 5)
    go = torch.randn(32, 64, 8192, device=dev)
    out_hip = ops.feature_interpolate(feature, index, weight)
    out_ref = torch_interpolate(feature, index, weight)
    row("interpolation bwd 32 x 64 x 2048 -> 8192", lambda: torch.autograd.grad(out_hip, feature, go, retain_graph=True),
        lambda: torch.autograd.grad(out_ref, feature, go, retain_graph=True), 5)

    rows.append("ordered backwards, the forms of one op in turn:")
    ordered_rows(ops, dev, calls, rows)
    head = ("pn2_bench: %s, median [min .. max] ms of %d eager calls (torch columns: fewer calls), HIP events"
            % (torch.cuda.get_device_name(0), calls))
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write("\n".join([head] + rows) + "\n")


def main():
    ordered_only = "--ordered" in sys.argv
    argv = [a for a in sys.argv if a != "--ordered"]
    if len(argv) > 1 and argv[1] == "--child":
        return child(argv[2], int(argv[3]), ordered_only)
    out_path = argv[1] if len(argv) > 1 else os.path.join(ROOT, "profiles", "pn2_bench.txt")
    calls = int(argv[2]) if len(argv) > 2 else 20
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", out_path, str(calls)]
                       + (["--ordered"] if ordered_only else []), timeout=TIME_LIMIT_S)
    sys.exit(r.returncode)


if __name__ == "__main__":
    main()
