"""Development-only (GPU box): the input stage of the MVPNet whole-scene test on the synthetic room of
tools/chunk_bench.py (200 000 points in 8 x 6 x 3 m, part of the floor plan thinned; chunks of 1.5 m, stride 0.5, margin
0.2, threshold 1000) with 100 synthetic frames of 120 x 160 on a 10 x 10 grid of cameras below the floor, 3 frames and 3
neighbours per chunk. A base point counts as seen by a frame when it lies within 1.5 m of the camera in x and y, so a
chunk chooses cameras under itself.

Two paths, for G in {1, 4, 16, 32} chunks per forward:
  parent   chunk_rgbd_inputs for every chunk, then chunk_groups (pad, collate): one chunk at a time, host-driven
  device   group_rgbd_inputs: G chunks per handful of launches, nothing read back
measured as the input stage alone (the generator is consumed, nothing is forwarded) and as the whole scene
(predict_whole_scene_grouped over the parent's inputs against predict_whole_scene_rgbd) with the frozen default PN2SSG fed
from a per-point feature table as in tools/pn2_ragged_bench.py ('knn_indices'[..., 0] picks the row).

Paths and settings alternate scene by scene in one process: 5 warm-up rounds, then `scenes` timed rounds (default 20).
Each scene lies between two HIP events after a device synchronisation, with the wall clock beside them (taken after the
synchronisation that ends the scene). The parent path is bound by the host, so the wall clock is the honest figure.
Reported: median [min .. max] milliseconds per scene.

Writes profiles/scene_inputs_bench.txt (or the path given).  usage: python tools/scene_inputs_bench.py [out.txt] [scenes]"""
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
one_chunk = mvkpconv.sub("dropin.mvpnet.test_mvpnet_3d")
grouped = mvkpconv.sub("dropin.mvpnet.whole_scene_grouped")
scene_inputs = mvkpconv.sub("dropin.mvpnet.whole_scene_inputs")
pn2ssg = mvkpconv.sub("dropin.mvpnet.models.pn2.pn2ssg")
dev = torch.device("cuda:0")
C, C_IN, MIN_NB_PTS = 20, 64, 2048
NF, H, W, NV, K, NB = 100, 120, 160, 3, 3, 5000
GROUPS = (1, 4, 16, 32)
ARGS = dict(chunk_size=(1.5, 1.5), stride=0.5, thresh=1000, margin=(0.2, 0.2))


class DirectFeatures(torch.nn.Module):
    """The 3D network fed from a per-point feature table: 'knn_indices' (B, N, k) holds a row per point in column 0."""

    def __init__(self, net_3d, table):
        super().__init__()
        self.net_3d, self.table = net_3d, table                         # table (C_IN, rows)

    def forward(self, batch):
        rows = batch["knn_indices"][..., 0]                             # (B, N); padded rows are 0, a valid row
        batch_3d = {"points": batch["points"], "feature": self.table[:, rows].transpose(0, 1).contiguous()}
        if "lengths" in batch:
            batch_3d["lengths"] = batch["lengths"]
        return self.net_3d(batch_3d)


def room_frames(points, rng):
    lo, hi = points.min(0), points.max(0)
    cam = np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]], np.float32)
    depth = rng.integers(900, 2100, size=(NF, H, W)).astype(np.int16)
    depth[rng.random((NF, H, W)) < 0.05] = 0                            # holes
    poses = np.tile(np.eye(4, dtype=np.float32), (NF, 1, 1))
    gx, gy = np.meshgrid(np.linspace(lo[0], hi[0], 10), np.linspace(lo[1], hi[1], 10), indexing="ij")
    poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = gx.reshape(-1), gy.reshape(-1), -1.0
    base = np.sort(rng.choice(len(points), NB, replace=False)).astype(np.int64)
    near = np.abs(points[base][:, None, :2] - poses[None, :, :2, 3]).max(axis=2) < 1.5
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return {"depth": t(depth), "images": t(rng.standard_normal((NF, H, W, 3)).astype(np.float32)), "poses": t(poses),
            "cam_matrix": cam, "base_point_ind": t(base), "pointwise_rgbd_overlap": t(near)}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "scene_inputs_bench.txt")
    scenes = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = 5
    points = chunk_ref.random_scene(0, 310000, ext=(8.0, 6.0, 3.0))[:200000]
    pts = torch.from_numpy(points).to(dev)
    indices, boxes = chunk_util.scene2chunks_legacy(pts, return_bbox=True, **ARGS)
    frames = room_frames(points, np.random.default_rng(0))
    sf = scene_inputs.SceneFrames(frames)

    torch.manual_seed(0)
    net_3d = pn2ssg.PN2SSG(C_IN, C).to(dev).eval()
    model = pn2ssg.freeze_inference(DirectFeatures(net_3d, torch.randn((C_IN, NV * H * W), device=dev))).eval()

    def parent_inputs():
        return (one_chunk.chunk_rgbd_inputs(pts, ind, box, frames, NV, k=K) for ind, box in zip(indices, boxes))

    def device_groups(g):
        return scene_inputs.group_rgbd_inputs(pts, indices, boxes, sf, NV, k=K, chunks_per_forward=g, min_nb_pts=MIN_NB_PTS)

    def consume(groups):
        for _ in groups:
            pass

    runs = {
        ("inputs", "parent"): lambda g: consume(grouped.chunk_groups(parent_inputs(), g, MIN_NB_PTS, dev)),
        ("inputs", "device"): lambda g: consume(device_groups(g)),
        ("scene", "parent"): lambda g: grouped.predict_whole_scene_grouped(model, pts, parent_inputs(), min_nb_pts=MIN_NB_PTS,
                                                                           chunks_per_forward=g),
        ("scene", "device"): lambda g: scene_inputs.predict_whole_scene_rgbd(model, pts, indices, boxes, sf, NV, k=K,
                                                                             min_nb_pts=MIN_NB_PTS, chunks_per_forward=g),
    }

    # the two paths give the same batches (the first group of 4 chunks, as bits) and the same scene
    np.random.seed(0)
    a = next(iter(grouped.chunk_groups(parent_inputs(), 4, MIN_NB_PTS, dev)))[0]
    np.random.seed(0)
    b = next(iter(device_groups(4)))[0]
    same = all(torch.equal(a[key].contiguous().view(torch.uint8), b[key].contiguous().view(torch.uint8)) for key in a)
    np.random.seed(0)
    pred_a, _ = runs["scene", "parent"](4)
    np.random.seed(0)
    pred_b, _ = runs["scene", "device"](4)
    differ = int((pred_a != pred_b).sum())

    device_ms = {key + (g,): [] for key in runs for g in GROUPS}
    wall_ms = {key + (g,): [] for key in runs for g in GROUPS}
    for it in range(warmup + scenes):
        for g in GROUPS:
            for key, run in runs.items():
                np.random.seed(0)                                       # the pad draws of sparse chunks
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                run(g)
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if it >= warmup:
                    device_ms[key + (g,)].append(e0.elapsed_time(e1))
                    wall_ms[key + (g,)].append(1e3 * (t1 - t0))

    def fmt(t):
        return "%9.3f [%9.3f .. %9.3f]" % (np.median(t), np.min(t), np.max(t))

    sizes = [len(i) for i in indices]
    lines = ["scene_inputs_bench: %d points, %d chunks of %d .. %d points (%d below min_nb_pts = %d), %d frames of %d x %d, %d "
             "base points, %d frames and %d neighbours per chunk; median [min .. max] ms per scene over %d scenes after %d "
             "warm-ups, paths and settings alternating. parent = chunk_rgbd_inputs + chunk_groups, device = group_rgbd_inputs. "
             "First group of 4 chunks bit-equal between the paths: %s; predictions of the scene at G = 4 that differ: %d"
             % (len(points), len(indices), min(sizes), max(sizes), sum(s < MIN_NB_PTS for s in sizes), MIN_NB_PTS, NF, H, W, NB,
                NV, K, scenes, warmup, same, differ)]
    for what, title in (("inputs", "input stage alone"), ("scene", "whole scene, frozen PN2SSG(%d, %d) stand-in" % (C_IN, C))):
        lines.append(title)
        for g in GROUPS:
            p, d = (what, "parent", g), (what, "device", g)
            lines.append("  G = %2d   wall clock: parent %s  device %s  parent / device %6.2f   |   HIP events: parent %s  device %s"
                         % (g, fmt(wall_ms[p]), fmt(wall_ms[d]), np.median(wall_ms[p]) / np.median(wall_ms[d]),
                            fmt(device_ms[p]), fmt(device_ms[d])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
