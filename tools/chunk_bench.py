"""Development-only (GPU box): what the MVPNet whole-scene test costs around the network on one synthetic room scene
(200 000 points in 8 x 6 x 3 m, part of the floor plan thinned; chunks of 1.5 m, stride 0.5, margin 0.2, threshold 1000;
20 classes), with table logits standing for the network:

  (a) chunking:  mvpnet.utils.chunk_util.scene2chunks_legacy(return_bbox=True) on the scene in HBM (csrc/chunk.hip),
  (b) vote:      WholeSceneVoter.add over all chunks, each chunk's logits a [20, ld] slice in HBM (ld > n),
  (c) finish:    WholeSceneVoter.finish with labels and an Evaluator (division, arg-max, confusion),

each against the NumPy restatement of the reference's own loop (tests/chunk_ref.py: chunk_util.py:4-53,
test_mvpnet_3d.py:141-178, evaluate_3d.py:19-36) on this host in the same call. The reference additionally copies every
chunk's logits to the host before its NumPy update; that copy is NOT in the host figures (they start from logits that
are already on the host), so the comparison favours the reference.

Device stages: median [min .. max] milliseconds between two HIP events after a device synchronisation (host work inside
a stage -- the corner list, the reads of the counts -- falls between its events). Host stages: time.perf_counter.
5 warm-ups; `calls` timed repeats of the device stages (default 20), `host_calls` of the host stages (default 5).
Writes profiles/chunk_bench.txt (or the path given).  usage: python tools/chunk_bench.py [out.txt] [calls] [host_calls]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvkpconv
import chunk_ref

chunk_util = mvkpconv.sub("dropin.mvpnet.utils.chunk_util")
evaluate_3d = mvkpconv.sub("dropin.mvpnet.evaluate_3d")
test_loop = mvkpconv.sub("dropin.mvpnet.test_mvpnet_3d")
dev = torch.device("cuda:0")
C = 20
ARGS = dict(chunk_size=(1.5, 1.5), stride=0.5, thresh=1000, margin=(0.2, 0.2))


def device_ms(fn, calls, warmup=5):
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


def host_ms(fn, calls):
    fn()
    out = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(out)), float(np.min(out)), float(np.max(out))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "chunk_bench.txt")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    host_calls = int(sys.argv[3]) if len(sys.argv) > 3 else 5
    points = chunk_ref.random_scene(0, 310000, ext=(8.0, 6.0, 3.0))[:200000]
    n = len(points)
    assert n == 200000
    rng = np.random.default_rng(1)
    labels = rng.integers(-1, C + 1, size=n).astype(np.int64)
    pts = torch.from_numpy(points).to(dev)
    lab = torch.from_numpy(labels).to(dev)

    indices, _ = chunk_util.scene2chunks_legacy(pts, return_bbox=True, **ARGS)
    want_indices, _ = chunk_ref.scene2chunks(points, **ARGS)
    assert len(indices) == len(want_indices) and all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(indices, want_indices))
    sizes = [len(i) for i in indices]
    table = chunk_ref.table_logits(2, C, [max(sizes) + 64])[0]
    table_dev = torch.from_numpy(table).to(dev)
    names = ["c%d" % i for i in range(C)]

    def dev_vote():
        voter = test_loop.WholeSceneVoter(n, C, dev)
        for ind in indices:
            voter.add(table_dev, ind)
        return voter

    def dev_finish():
        # a finished voter cannot be finished again: the stage is timed on a fresh copy of the sums each call
        voter = test_loop.WholeSceneVoter(n, C, dev)
        voter.logit_sum.copy_(state[0])
        voter.num_pred.copy_(state[1])
        return voter

    voter = dev_vote()
    state = (voter.logit_sum.clone(), voter.num_pred.clone())
    fresh = []

    def finish_stage():
        return fresh.pop().finish(lab, evaluate_3d.Evaluator(names))

    def timed_finish(calls_, warmup=5):
        out = []
        for it in range(warmup + calls_):
            fresh.append(dev_finish())
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            finish_stage()
            e1.record()
            torch.cuda.synchronize()
            if it >= warmup:
                out.append(e0.elapsed_time(e1))
        return float(np.median(out)), float(np.min(out)), float(np.max(out))

    t_chunk = device_ms(lambda: chunk_util.scene2chunks_legacy(pts, return_bbox=True, **ARGS), calls)
    t_vote = device_ms(dev_vote, calls)
    t_finish = timed_finish(calls)

    host_chunks = [(table, ind) for ind in want_indices]
    h_chunk = host_ms(lambda: chunk_ref.scene2chunks(points, **ARGS), host_calls)

    def host_vote():
        sums = np.zeros([n, C], dtype=np.float32)
        visits = np.zeros(n, dtype=np.uint8)
        for logits, ind in host_chunks:
            sums[ind] += logits.T[:len(ind)]
            visits[ind] += 1
        return sums, visits

    h_vote = host_ms(host_vote, host_calls)
    sums, visits = host_vote()

    def host_finish():
        mean = sums / np.maximum(visits[:, np.newaxis], 1)
        pred = np.argmax(mean, axis=1)
        pred[np.nonzero(visits == 0)[0]] = C
        return mean, pred, chunk_ref.evaluator_update(np.zeros((C, C)), pred, labels, C)

    h_finish = host_ms(host_finish, host_calls)

    # the two routes computed the same thing
    mean, pred, conf = host_finish()
    ev = evaluate_3d.Evaluator(names)
    got_pred, got_mean = dev_vote().finish(lab, ev)
    assert np.array_equal(got_pred.cpu().numpy(), pred) and np.array_equal(got_mean.cpu().numpy(), mean)
    assert np.array_equal(ev.confusion_matrix, conf)

    lines = ["chunk_bench: %d points, %d corners kept of %d, chunk sizes %d .. %d (sum %d), %d classes; median [min .. max] ms; "
             "%d device calls, %d host calls" % (n, len(indices), len(chunk_ref.corners(points)), min(sizes), max(sizes),
                                                  sum(sizes), C, calls, host_calls)]
    for tag, d, h in (("(a) chunking (indices + bboxes)", t_chunk, h_chunk), ("(b) vote over all chunks", t_vote, h_vote),
                      ("(c) finish (mean, arg-max, confusion)", t_finish, h_finish)):
        lines.append("%-40s device %9.3f [%9.3f .. %9.3f]   NumPy on the host %10.3f [%10.3f .. %10.3f]   host / device %7.1f"
                     % ((tag,) + d + h + (h[0] / d[0],)))
    tot_d, tot_h = t_chunk[0] + t_vote[0] + t_finish[0], h_chunk[0] + h_vote[0] + h_finish[0]
    lines.append("%-40s device %9.3f                              NumPy on the host %10.3f                              host / device %7.1f"
                 % ("sum of the medians", tot_d, tot_h, tot_h / tot_d))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
