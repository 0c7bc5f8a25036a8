"""Development-only (GPU box): one training batch of the MVPNet baseline's inputs: B = 32 items of 32 resident
synthetic scenes (150 000 points in 8 x 6 x 3 m, one point in ten unlabeled; 125 frames of 120 x 160 on a 25 x 5 grid of
cameras below the floor; 5 000 base points, seen by a frame when within 1.5 m of its camera in x and y), nb_pts 8 192,
3 frames and 3 neighbours per item, flip 0.5, z rotation +-180 degrees, 10 tries.

Three paths over the same 32 scenes:
  device   train_chunk_batch: the five library calls and the k-NN behind one upload, nothing read back. Timed as a whole
           (HIP events and wall clock) and stage by stage (HIP events between the calls, the same draws)
  parent   what the parent commit offers, one item at a time: a torch mask per try with its labeled share read back,
           nonzero, torch.randperm for the resample, chunk_rgbd_inputs on the whole chunk and a gather of the sampled
           rows; no flip and no rotation (they cannot be applied before the k-NN's pixel numbering from outside)
  host     the NumPy restatement of tests/train_inputs_ref.py on 16 threads, its k-NN replaced by scikit-learn's ball
           tree (what the reference uses) where scikit-learn is importable

Paths alternate round by round in one process: 3 warm-up rounds, then `rounds` timed ones (default 20; the host path
runs every fifth round). Reported: median [min .. max] milliseconds per batch.

Writes profiles/train_inputs_bench.txt (or the path given).  usage: python tools/train_inputs_bench.py [out.txt] [rounds]"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mvkpconv
import train_inputs_ref as ref

ops = mvkpconv.sub("ops")
one_chunk = mvkpconv.sub("dropin.mvpnet.test_mvpnet_3d")
train_inputs = mvkpconv.sub("dropin.mvpnet.train_inputs")
dev = torch.device("cuda:0")
B, N, NF, H, W, NV, K, NB, NB_PTS, TRIES = 32, 150000, 125, 120, 160, 3, 3, 5000, 8192, 10
FLIP, Z_ROT, SIZE, MARGIN, THRESH = 0.5, (-180, 180), (1.5, 1.5), (0.2, 0.2), 0.3
EXT = (8.0, 6.0, 3.0)


def make_scene(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    points = torch.rand((N, 3), generator=g, device=dev) * torch.tensor(EXT, device=dev)
    labels = torch.randint(0, 20, (N,), generator=g, device=dev)
    labels[torch.rand((N,), generator=g, device=dev) < 0.1] = -100
    depth = torch.randint(900, 2100, (NF, H, W), generator=g, device=dev).to(torch.int16)
    depth[torch.rand((NF, H, W), generator=g, device=dev) < 0.05] = 0
    poses = torch.eye(4, device=dev).repeat(NF, 1, 1)
    gx, gy = torch.meshgrid(torch.linspace(0, EXT[0], 25, device=dev), torch.linspace(0, EXT[1], 5, device=dev), indexing="ij")
    poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = gx.reshape(-1), gy.reshape(-1), -1.0
    base = torch.sort(torch.randperm(N, generator=g, device=dev)[:NB]).values
    near = (points[base][:, None, :2] - poses[None, :, :2, 3]).abs().amax(dim=2) < 1.5
    return {"points": points, "seg_label": labels, "depth": depth, "poses": poses, "base_point_ind": base,
            "images": torch.randn((NF, H, W, 3), generator=g, device=dev), "pointwise_rgbd_overlap": near,
            "cam_matrix": np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]], np.float32)}


def staged_device_batch(ts, ids, draws, events):
    """train_chunk_batch's calls with an event after each stage (the module's own function is timed as a whole)."""
    res = ts.resident
    centers, seeds, flips, angles = draws
    sizes = ts.num_points[ids]
    row_off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rot = np.stack([train_inputs.z_rotation(a) for a in angles]).reshape(B, 9)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)
    events[0].record()
    sid, cen, sd, off = up(ids), up(centers), up(seeds), up(row_off[:B])
    samp, rot_d, fl = up(np.arange(B + 1, dtype=np.int64) * NB_PTS), up(rot), up(flips)
    events[1].record()
    _, chosen, box, rows, row_len = ops.train_chunk_pick(res, sid, cen, off, int(row_off[B]), SIZE, MARGIN, THRESH,
                                                         max_points=int(sizes.max()))
    events[2].record()
    sample_rows, _ = ops.train_chunk_resample(rows, off, row_len, sd, NB_PTS)
    events[3].record()
    sel = ops.train_select_frames(res, sid, rows, off, row_len, NV)
    events[4].record()
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(res, sel, sid, box, flips=fl, rot=rot_d)
    events[5].record()
    queries, knn = ops.chunk_knn_many(res.points, sample_rows.view(-1), samp[:B], samp, np.full(B, NB_PTS, np.int64), keys,
                                      image_mask, k=K)
    events[6].record()
    ops.train_batch_rows(queries, res.labels, sample_rows, rot=rot_d)
    events[7].record()


STAGES = ("upload", "pick", "resample", "select_frames", "unproject", "knn", "batch_rows")


def parent_batch(scenes, ids, centers):
    size = torch.tensor(SIZE, device=dev)
    margin = torch.tensor(MARGIN, device=dev)
    out = []
    for b, s in enumerate(ids):
        sc = scenes[s]
        pts, lab = sc["points"], sc["seg_label"]
        xy = pts[:, :2]
        mask = None
        for c in centers[b]:
            lo, hi = (xy[c] - 0.5 * size) - margin, (xy[c] + 0.5 * size) + margin
            m = ((xy >= lo) & (xy <= hi)).all(dim=1)
            picked = lab[m]
            if picked.numel() and float((picked >= 0).float().mean()) >= THRESH:       # a read back per try
                mask = m
                break
        if mask is None:
            lo, hi, mask = xy.min(0).values - margin, xy.max(0).values + margin, torch.ones_like(lab, dtype=torch.bool)
        ind = mask.nonzero().squeeze(1)
        box = torch.cat([lo, lo.new_zeros(1), hi, hi.new_zeros(1)]).cpu().numpy()
        data = one_chunk.chunk_rgbd_inputs(pts, ind, box, sc, NV, k=K)
        n = ind.numel()
        choice = torch.randperm(n, device=dev)[:NB_PTS] if n >= NB_PTS else \
            torch.cat([torch.arange(n, device=dev), torch.randint(n, (NB_PTS - n,), device=dev)])
        out.append((data["points"][..., choice], lab[ind[choice]], data["knn_indices"][choice], data["images"],
                    data["image_xyz"], data["image_mask"]))
    return out


def sklearn_knn(queries32, keys64, valid, k):
    from sklearn.neighbors import NearestNeighbors
    ind = np.nonzero(valid)[0]
    out = np.full((len(queries32), k), -1, np.int64)
    if len(ind) >= k:
        out[:] = ind[NearestNeighbors(n_neighbors=k, algorithm="ball_tree").fit(keys64[ind]).kneighbors(queries32)[1]]
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "train_inputs_bench.txt")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = 3
    scenes = [make_scene(s) for s in range(B)]
    ts = train_inputs.TrainScenes(scenes)
    ids = np.arange(B, dtype=np.int64)
    try:
        import sklearn  # noqa: F401
        ref.knn, host_knn = sklearn_knn, "scikit-learn ball tree"
    except ImportError:
        host_knn = "brute force"
    host_scenes = [{k: (v.cpu().numpy() if isinstance(v, torch.Tensor) else v) for k, v in sc.items()} for sc in scenes]
    pool = ThreadPoolExecutor(16)

    def draws_for(round_):
        np.random.seed(round_)
        return train_inputs.draw_items(ts.num_points[ids], NV, FLIP, Z_ROT, TRIES)

    def host_batch(draws):
        centers, seeds, flips, angles = draws
        return list(pool.map(lambda b: ref.item(host_scenes[b], centers[b], NB_PTS, NV, K, seed=seeds[b], flips=flips[b],
                                                rot=train_inputs.z_rotation(angles[b]), chunk_size=SIZE,
                                                chunk_thresh=THRESH, chunk_margin=MARGIN), range(B)))

    # the device batch is the restatement's, bit for bit (items 0 and 1, with the host path's k-NN)
    d0 = draws_for(0)
    got = train_inputs.train_chunk_batch(ts, ids, NB_PTS, NV, k=K, chunk_size=SIZE, chunk_thresh=THRESH, chunk_margin=MARGIN,
                                         flip=FLIP, z_rot=Z_ROT, tries=TRIES, draws=d0)
    same = True
    for b in (0, 1):
        want = ref.item(host_scenes[b], d0[0][b], NB_PTS, NV, K, seed=d0[1][b], flips=d0[2][b],
                        rot=train_inputs.z_rotation(d0[3][b]))
        same &= all(np.array_equal(got[key][b].cpu().numpy().view(np.uint8), np.ascontiguousarray(want[key]).view(np.uint8))
                    for key in ("points", "seg_label", "images", "image_xyz", "knn_indices"))
    tries = got["chunk_try"].cpu().numpy()

    total_ev, total_wall, stage_ms = [], [], {s: [] for s in STAGES}
    parent_ev, parent_wall, host_wall = [], [], []
    for it in range(warmup + rounds):
        draws = draws_for(it)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        train_inputs.train_chunk_batch(ts, ids, NB_PTS, NV, k=K, chunk_size=SIZE, chunk_thresh=THRESH, chunk_margin=MARGIN,
                                       flip=FLIP, z_rot=Z_ROT, tries=TRIES, draws=draws)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        events = [torch.cuda.Event(enable_timing=True) for _ in range(8)]
        staged_device_batch(ts, ids, draws, events)
        torch.cuda.synchronize()
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t2 = time.perf_counter()
        p0.record()
        parent_batch(scenes, ids, draws[0])
        p1.record()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        if it >= warmup:
            total_ev.append(e0.elapsed_time(e1))
            total_wall.append(1e3 * (t1 - t0))
            for i, s in enumerate(STAGES):
                stage_ms[s].append(events[i].elapsed_time(events[i + 1]))
            parent_ev.append(p0.elapsed_time(p1))
            parent_wall.append(1e3 * (t3 - t2))
            if (it - warmup) % 5 == 0:
                t4 = time.perf_counter()
                host_batch(draws)
                host_wall.append(1e3 * (time.perf_counter() - t4))

    def fmt(t):
        return "%9.3f [%9.3f .. %9.3f]" % (np.median(t), np.min(t), np.max(t))

    lines = ["train_inputs_bench: B = %d items of %d scenes of %d points, %d frames of %d x %d and %d base points each; nb_pts "
             "%d, %d frames and %d neighbours per item, flip %.1f, z_rot %s, %d tries (items that fell back to the whole scene "
             "in round 0: %d). median [min .. max] ms per batch over %d rounds after %d warm-ups, paths alternating. Items 0 and "
             "1 of the device batch bit-equal to the restatement: %s"
             % (B, B, N, NF, H, W, NB, NB_PTS, NV, K, FLIP, Z_ROT, TRIES, int((tries < 0).sum()), rounds, warmup, same),
             "  device  train_chunk_batch            wall clock %s   HIP events %s" % (fmt(total_wall), fmt(total_ev))]
    for s in STAGES:
        lines.append("            %-14s HIP events %s" % (s, fmt(stage_ms[s])))
    lines.append("  parent  mask / nonzero / randperm / chunk_rgbd_inputs, one item at a time (no flip, no rotation)")
    lines.append("                                       wall clock %s   HIP events %s" % (fmt(parent_wall), fmt(parent_ev)))
    lines.append("  host    NumPy restatement on 16 threads, k-NN by %s (%d rounds)" % (host_knn, len(host_wall)))
    lines.append("                                       wall clock %s" % fmt(host_wall))
    lines.append("  parent / device (wall clock) %.2f   host / device (wall clock) %.2f"
                 % (np.median(parent_wall) / np.median(total_wall), np.median(host_wall) / np.median(total_wall)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
