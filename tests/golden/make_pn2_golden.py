#!/usr/bin/env python3
"""Generate tests/golden/g15_pn2_ops.npz and g16_pn2ssg.npz from the REFERENCE ITSELF (build container, CPU only).

Run from the repo root:   python tests/golden/make_pn2_golden.py

The reference's PointNet++ ops are CUDA extensions that cannot be built here, but the reference ships restatements of
them in its own tests (mvpnet/ops/tests/*.py). This script takes those FUNCTIONS out of the reference's test files at
generation time (the files themselves import the CUDA extensions at their head and cannot be imported) and executes them:

g15_pn2_ops    inputs drawn as the reference's tests draw them (same seeds and calls, reduced shapes where theirs are
               large) in float64 and float32, and the outputs of farthest_point_sample_np, ball_query_np,
               ball_query_distance_np, torch.topk on the reference's bpdist2 distance matrix (test_knn_distance.py) and
               feature_interpolate_torch (forward, and the gradient of its sum weighted by a stored tensor).
g16_pn2ssg     the reference's class texts of mvpnet/models/pn2/modules.py and pn2ssg.py, executed on torch-CPU with the
               five CUDA ops they import SUBSTITUTED by those restatements:
                   farthest_point_sample -> farthest_point_sample_np      ball_query -> ball_query_np
                   group_points -> group_points_torch                     knn_distance -> knn_distance_torch
                   feature_interpolate -> feature_interpolate_torch
               (common.nn, common.nn.functional.batch_index_select and common.nn.init.xavier_uniform are the
               reference's own). PN2SSG(in_channels=4, num_classes=5, sa_channels=((16,16,32),(32,32,64)),
               num_centroids=(64,16), radius=(0.2,0.4), max_neighbors=(8,8), fp_channels=((32,32),(32,16)),
               fp_neighbors=(3,3), seg_channels=(16,), dropout_prob=0.0) on B=2, N=256 points of the unit cube: state
               dict, inputs, eval-mode and train-mode logits in float32 and float64, the gradients of
               logits.square().mean() (train mode) in both, and the indices every op produced. The float32 and
               float64 runs must produce identical indices (asserted; pick another seed otherwise).

Only DATA is written; no reference source text.
"""
import ast
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden")
REFROOT = "/root/reference"
sys.dont_write_bytecode = True


def take(rel_path, kinds=(ast.FunctionDef, ast.ClassDef), skip=()):
    """Compiled module holding only the function / class definitions of a reference file (its imports dropped)."""
    path = os.path.join(REFROOT, rel_path)
    tree = ast.parse(open(path).read(), path)
    tree.body = [n for n in tree.body if isinstance(n, kinds) and n.name not in skip]
    return compile(tree, path, "exec")


def namespace(rel_path, **given):
    ns = dict(np=np, torch=torch, nn=torch.nn, **given)
    exec(take(rel_path, skip=("test", "test_ball_query", "test_ball_query_distance", "test_PN2SSG")), ns)
    return ns


def save(name, arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrs)
    print("wrote", path, os.path.getsize(path), "bytes,", len(arrs), "arrays")


FPS_CASES = ((2, 3, 256, 32, True), (2, 2, 256, 32, True), (3, 3, 257, 33, True), (3, 3, 257, 33, False))
BQ_CASES = ((2, 64, 128, 0.1, 32, True), (3, 65, 129, 0.1, 32, True), (3, 65, 129, 10.0, 32, True),
            (3, 65, 129, 0.1, 32, False))
KNN_CASES = ((2, 64, 128, True), (3, 65, 129, True), (3, 65, 129, False), (3, 31, 63, True))
INTERP_CASES = ((2, 8, 32, 64), (3, 9, 33, 65))


def g15():
    fps = namespace("mvpnet/ops/tests/test_fps.py")
    bq = namespace("mvpnet/ops/tests/test_ball_query.py")
    knn = namespace("mvpnet/ops/tests/test_knn_distance.py")
    itp = namespace("mvpnet/ops/tests/test_interpolate.py")
    arrs = {}
    for i, (b, c, n, m, tr) in enumerate(FPS_CASES):
        np.random.seed(0)
        pts = np.random.rand(b, c, n) if tr else np.random.rand(b, n, c)
        for tag, dt in (("f64", np.float64), ("f32", np.float32)):
            p = pts.astype(dt)
            arrs["fps%d_%s_points" % (i, tag)] = p
            arrs["fps%d_%s_index" % (i, tag)] = fps["farthest_point_sample_np"](p, m, transpose=tr).astype(np.int64)
        arrs["fps%d_transpose" % i] = np.array(tr)
    for i, (b, n1, n2, r, k, tr) in enumerate(BQ_CASES):
        np.random.seed(0)
        if tr:
            key = np.random.randn(b, 3, n2)
            query = np.array([p[:, np.random.choice(n2, n1, replace=False)] for p in key])
        else:
            key = np.random.randn(b, n2, 3)
            query = np.array([p[np.random.choice(n2, n1, replace=False)] for p in key])
        for tag, dt in (("f64", np.float64), ("f32", np.float32)):
            q, ky = query.astype(dt), key.astype(dt)
            idx = bq["ball_query_np"](q, ky, r, k, transpose=tr)
            idx2, dist = bq["ball_query_distance_np"](q, ky, r, k, transpose=tr)
            assert np.array_equal(idx, idx2)
            arrs["bq%d_%s_query" % (i, tag)], arrs["bq%d_%s_key" % (i, tag)] = q, ky
            arrs["bq%d_%s_index" % (i, tag)] = idx.astype(np.int64)
            arrs["bq%d_%s_distance" % (i, tag)] = dist            # float32: the restatement's own output dtype
        arrs["bq%d_radius_k_transpose" % i] = np.array([r, k, int(tr)], np.float64)
    for i, (b, n1, n2, tr) in enumerate(KNN_CASES):
        np.random.seed(0)
        if tr:
            q, ky = np.random.randn(b, 3, n1).astype(np.float32), np.random.randn(b, 3, n2).astype(np.float32)
        else:
            q, ky = np.random.randn(b, n1, 3).astype(np.float32), np.random.randn(b, n2, 3).astype(np.float32)
        for tag, dt in (("f32", np.float32), ("f64", np.float64)):
            idx, dist = knn["knn_distance_torch"](torch.tensor(q.astype(dt)), torch.tensor(ky.astype(dt)), 3, transpose=tr)
            arrs["knn%d_%s_query" % (i, tag)], arrs["knn%d_%s_key" % (i, tag)] = q.astype(dt), ky.astype(dt)
            arrs["knn%d_%s_index" % (i, tag)] = idx.numpy().astype(np.int64)
            arrs["knn%d_%s_distance" % (i, tag)] = dist.numpy()
        arrs["knn%d_transpose" % i] = np.array(tr)
    for i, (b, c, n1, n2) in enumerate(INTERP_CASES):
        torch.manual_seed(0)
        feature = torch.randn(b, c, n1).double()
        index = torch.randint(0, n1, [b, n2, 3]).long()
        weight = torch.rand(b, n2, 3).double()
        weight = weight / weight.sum(dim=2, keepdim=True)
        gout = torch.randn(b, c, n2).double()
        f = feature.clone().requires_grad_(True)
        out = itp["feature_interpolate_torch"](f, index, weight)
        (out * gout).sum().backward()
        arrs.update({"itp%d_feature" % i: feature.numpy(), "itp%d_index" % i: index.numpy(), "itp%d_weight" % i: weight.numpy(),
                     "itp%d_grad_out" % i: gout.numpy(), "itp%d_out" % i: out.detach().numpy(),
                     "itp%d_grad_feature" % i: f.grad.numpy()})
    save("g15_pn2_ops", arrs)


NET_KW = dict(in_channels=4, num_classes=5, sa_channels=((16, 16, 32), (32, 32, 64)), num_centroids=(64, 16),
              radius=(0.2, 0.4), max_neighbors=(8, 8), fp_channels=((32, 32), (32, 16)), fp_neighbors=(3, 3),
              seg_channels=(16,), dropout_prob=0.0)


def g16(seed=16):
    sys.path.insert(0, REFROOT)
    from common.nn import SharedMLP, SharedMLPDO
    from common.nn.functional import batch_index_select
    from common.nn.init import xavier_uniform
    fps = namespace("mvpnet/ops/tests/test_fps.py")
    bq = namespace("mvpnet/ops/tests/test_ball_query.py")
    knn = namespace("mvpnet/ops/tests/test_knn_distance.py")
    itp = namespace("mvpnet/ops/tests/test_interpolate.py")
    grp = namespace("mvpnet/ops/tests/test_group_points.py")
    log = {}

    def note(kind, value):
        log.setdefault(kind, []).append(value.numpy().copy())
        return value

    def farthest_point_sample(points, num_centroids, transpose=True):
        return note("fps", torch.from_numpy(np.asarray(fps["farthest_point_sample_np"](
            points.detach().numpy(), num_centroids, transpose=transpose), np.int64)))

    def ball_query(query, key, radius, max_neighbors, transpose=True):
        return note("bq", torch.from_numpy(np.asarray(bq["ball_query_np"](
            query.detach().numpy(), key.detach().numpy(), radius, max_neighbors, transpose=transpose), np.int64)))

    def knn_distance(query, key, k, transpose=True):
        index, distance = knn["knn_distance_torch"](query, key, k, transpose=transpose)
        note("knn", index)
        return index, distance

    mods = namespace("mvpnet/models/pn2/modules.py", SharedMLP=SharedMLP, batch_index_select=batch_index_select,
                     farthest_point_sample=farthest_point_sample, group_points=grp["group_points_torch"],
                     ball_query=ball_query, knn_distance=knn_distance,
                     feature_interpolate=itp["feature_interpolate_torch"])
    net_ns = namespace("mvpnet/models/pn2/pn2ssg.py", SharedMLPDO=SharedMLPDO, xavier_uniform=xavier_uniform,
                       SetAbstraction=mods["SetAbstraction"], FeaturePropagation=mods["FeaturePropagation"])
    torch.manual_seed(seed)
    rng = np.random.default_rng(seed)
    net = net_ns["PN2SSG"](**NET_KW)
    with torch.no_grad():                                   # BatchNorm away from its initial values, so eval mode tests something
        for m in net.modules():
            if isinstance(m, torch.nn.modules.batchnorm._BatchNorm):
                m.weight.copy_(torch.from_numpy(1 + 0.1 * rng.standard_normal(m.weight.shape)).float())
                m.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_mean.copy_(torch.from_numpy(0.1 * rng.standard_normal(m.bias.shape)).float())
                m.running_var.copy_(torch.from_numpy(1 + 0.1 * np.abs(rng.standard_normal(m.bias.shape))).float())
        net.seg_logit.bias.copy_(torch.from_numpy(0.1 * rng.standard_normal(net.seg_logit.bias.shape)).float())
    state = {k: v.clone() for k, v in net.state_dict().items()}
    points = torch.from_numpy(rng.random((2, 3, 256)).astype(np.float32))
    feature = torch.from_numpy(rng.standard_normal((2, 4, 256)).astype(np.float32))
    arrs = {"points": points.numpy(), "feature": feature.numpy()}
    for k, v in state.items():
        arrs["sd/" + k] = v.numpy()
    indices = {}
    for tag, dt in (("f32", torch.float32), ("f64", torch.float64)):
        net.load_state_dict(state)
        net.to(dt)
        batch = {"points": points.to(dt), "feature": feature.to(dt)}
        log.clear()
        net.eval()
        with torch.no_grad():
            arrs["logit_eval_" + tag] = net(batch)["seg_logit"].numpy()
        eval_log = {k: [a.copy() for a in v] for k, v in log.items()}
        log.clear()
        net.train()
        net.zero_grad()
        out = net(batch)["seg_logit"]
        out.square().mean().backward()
        arrs["logit_train_" + tag] = out.detach().numpy()
        for name, p in net.named_parameters():
            arrs["grad_%s/%s" % (tag, name)] = p.grad.numpy().copy()
        for kind in log:
            assert all(np.array_equal(a, b) for a, b in zip(log[kind], eval_log[kind]))
        indices[tag] = {k: [a.copy() for a in v] for k, v in log.items()}
        net.float()
    for kind in ("fps", "bq", "knn"):
        assert len(indices["f32"][kind]) == 2
        for lv in range(2):
            a, b = indices["f32"][kind][lv], indices["f64"][kind][lv]
            assert np.array_equal(a, b), "float32 and float64 %s indices differ at call %d: pick another seed" % (kind, lv)
            arrs["%s_%d" % (kind, lv)] = a
    save("g16_pn2ssg", arrs)


if __name__ == "__main__":
    torch.set_num_threads(4)
    g15()
    g16()
