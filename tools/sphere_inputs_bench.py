"""Development-only (GPU box): one batch of the KPFCNN networks' sphere inputs: 5 spheres of in_radius 1.2 m
(about 20 000 points each) with 5 views of 120 x 160 -- the reference's own batch shape -- from 5 resident synthetic
scenes (400 000 points in 8 x 6 x 3 m, 5 000 potential points, 60 frames on a 12 x 5 grid of cameras below the floor,
5 000 base points, seen by a frame when within 1.5 m of its camera in x and y), 3 neighbours, flip 0.5, 'vertical'
rotation, anisotropic scale, noise.

Comparison 1, two paths over the same scenes, each with its own potentials from the same start:
  device   sphere_batch: the pick, two member passes, the frame choice, the unprojection, the ragged k-NN and the row kernel
           behind one upload, nothing read back. Timed as a whole (HIP events and wall clock) and stage by stage (HIP events
           between the calls, the same draws)
  parent   what the parent commit offers, one sphere at a time: PotentialSphereSampler.pick() (three values read back and a
           count per ball query), torch.isin + voting.select_frames, ops.unproject_depth, ops.knn_pixels, and torch ops for
           the flip, the centring, the augmentation, the features and the stacking
Comparison 2, on the items of one device batch (rows, q_off, keys, masks):
  ragged   mvk_knn_f64_ragged, one call, lengths on the device
  B calls  mvk_knn_f64 per item (ops.knn_pixels on the gathered queries), the host given the lengths for free

Paths alternate round by round in one process: 3 warm-up rounds, then `rounds` timed ones (default 20). Reported: median
[min .. max] milliseconds. A path is called faster only when its maximum lies below the other's minimum.

Writes profiles/sphere_inputs_bench.txt (or the path given).  usage: python tools/sphere_inputs_bench.py [out.txt] [rounds]"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import mvkpconv

ops = mvkpconv.sub("ops")
si = mvkpconv.sub("dropin.datasets.sphere_inputs")
picking = mvkpconv.sub("dropin.datasets.sphere_picking")
voting = mvkpconv.sub("dropin.utils.voting")
dev = torch.device("cuda:0")
S, B, N, NPOT, NF, H, W, NV, K, NB = 5, 5, 400000, 5000, 60, 120, 160, 5, 3, 5000
R_IN, MARGIN, FLIP, CAP = 1.2, 0.1, 0.5, 160000
EXT = (8.0, 6.0, 3.0)


class Cfg(object):
    in_radius = R_IN
    augment_rotation = 'vertical'
    augment_scale_anisotropic = True
    augment_scale_min, augment_scale_max = 0.9, 1.1
    augment_symmetries = [True, False, False]
    augment_noise, augment_color = 0.005, 0.7
    early_fusion, in_features_dim = True, 66


def make_scene(seed):
    g = torch.Generator(device=dev).manual_seed(seed)
    points = torch.rand((N, 3), generator=g, device=dev) * torch.tensor(EXT, device=dev)
    depth = torch.randint(900, 2100, (NF, H, W), generator=g, device=dev).to(torch.int16)
    depth[torch.rand((NF, H, W), generator=g, device=dev) < 0.05] = 0
    poses = torch.eye(4, device=dev).repeat(NF, 1, 1)
    gx, gy = torch.meshgrid(torch.linspace(0, EXT[0], 12, device=dev), torch.linspace(0, EXT[1], 5, device=dev), indexing="ij")
    poses[:, 0, 3], poses[:, 1, 3], poses[:, 2, 3] = gx.reshape(-1), gy.reshape(-1), -1.0
    base = torch.sort(torch.randperm(N, generator=g, device=dev)[:NB]).values
    near = (points[base][:, None, :2] - poses[None, :, :2, 3]).abs().amax(dim=2) < 1.5
    inner = ((points > 1.2) & (points < torch.tensor(EXT, device=dev) - 1.2))[:, :2].all(1).nonzero().squeeze(1)
    pot = points[inner[torch.randperm(inner.numel(), generator=g, device=dev)[:NPOT]]].contiguous()
    return {"points": points, "colors": torch.rand((N, 3), generator=g, device=dev),
            "labels": torch.randint(0, 20, (N,), generator=g, device=dev), "pot_points": pot, "depth": depth, "poses": poses,
            "base_point_ind": base, "images": torch.randn((NF, H, W, 3), generator=g, device=dev),
            "pointwise_rgbd_overlap": near, "cam_matrix": np.array([[60.0, 0, W / 2], [0, 60.0, H / 2], [0, 0, 1]], np.float32)}


STAGES = ("upload", "pick", "members", "mask members", "select_frames", "unproject", "knn ragged", "batch_rows + features")


def staged_device_batch(ss, draws, noise, events):
    """sphere_batch's calls with an event after each stage (the module's own function is timed as a whole)."""
    res, sres = ss.resident, ss.sphere
    aug = [si.augmentation_of(Cfg, d) for d in draws]
    big = np.finfo(np.float32).max
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).pin_memory().to(dev, non_blocking=True)
    events[0].record()
    R_d, scale_d = up(np.stack([a[0] for a in aug]).reshape(B, 9)), up(np.stack([a[1] for a in aug]))
    keep_d = up(np.array([1.0 if d['keep_color'] else 0.0 for d in draws], np.float32))
    box_d = up(np.tile(np.array([-big, -big, big, big], np.float32), (B, 1)))
    flips_d = up(np.stack([d['flip'] for d in draws]).astype(np.uint8))
    events[1].record()
    cloud, point, centers, _, num = ops.sphere_pick(sres, R_IN, 1 << 40, B)
    events[2].record()
    status = torch.zeros((2,), device=dev, dtype=torch.int32)
    rows, q_off, _ = ops.sphere_members(res, cloud, centers, R_IN, CAP, status=status[0:1])
    events[3].record()
    mask_rows, mask_off, _ = ops.sphere_members(res, cloud, centers, R_IN + MARGIN, 2 * CAP, status=status[1:2])
    events[4].record()
    sel = ops.sphere_select_frames(res, cloud, mask_rows, mask_off, NV)
    events[5].record()
    keys, image_xyz, image_mask, images, num_valid = ops.train_unproject(res, sel, cloud, box_d, flips=flips_d)
    events[6].record()
    knn = ops.knn_f64_ragged(res.points, rows, q_off, keys, image_mask, k=K)
    events[7].record()
    r = ops.sphere_batch_rows(sres, cloud, centers, rows, q_off, R_d, scale_d, keep_d, knn, NV * H * W, noise=noise)
    si.stacked_3d_features(Cfg, r['colors'], r['world'])
    events[8].record()
    return rows, q_off, keys, image_mask, knn


def parent_batch(scenes, sampler, draws, noise):
    """One sphere at a time with what the parent commit has; the same outputs as the device batch."""
    out, at = [], 0
    for b in range(B):
        p = sampler.pick()
        sc = scenes[p["cloud_ind"]]
        inds, c64 = p["input_inds"], torch.from_numpy(p["center"]).to(dev)
        inside = torch.isin(sc["base_point_ind"], p["mask_inds"])
        sel = voting.select_frames(sc["pointwise_rgbd_overlap"][inside], NV)
        sel_d = torch.tensor(sel, device=dev)
        xyz, valid = ops.unproject_depth(sc["depth"][sel_d], sc["cam_matrix"], sc["poses"][sel_d])
        images = sc["images"][sel_d]
        fl = torch.from_numpy(np.asarray(draws[b]['flip'])).to(dev)
        xyz = torch.where(fl[:, None, None, None], xyz.flip(2), xyz)
        valid = torch.where(fl[:, None, None], valid.flip(2), valid)
        images = torch.where(fl[:, None, None, None], images.flip(2), images)
        world = sc["points"][inds]
        knn = ops.knn_pixels(world, xyz, valid, k=K)
        R, scale = si.augmentation_of(Cfg, draws[b])
        x = (world.double() - c64).float()
        R_d = torch.from_numpy(R).to(dev)
        aug = ((x[:, 0:1] * R_d[0] + x[:, 1:2] * R_d[1]) + x[:, 2:3] * R_d[2]) * torch.from_numpy(scale).to(dev) \
            + noise[at:at + inds.numel()]
        back = (aug.double() + c64).float()
        colors = sc["colors"][inds] * (1.0 if draws[b]['keep_color'] else 0.0)
        feats = si.stacked_3d_features(Cfg, colors, back)
        out.append((aug, feats, sc["labels"][inds], inds, world, images.permute(0, 3, 1, 2).contiguous(), xyz.float(), valid,
                    knn, knn + b * NV * H * W))
        at += inds.numel()
    return [torch.cat([o[i] for o in out]) for i in (0, 1, 2, 3, 4, 8, 9)] + [torch.stack([o[i] for o in out]) for i in (5, 6, 7)]


def fmt(t):
    t = np.asarray(t)
    return "%9.3f [%9.3f .. %9.3f]" % (np.median(t), t.min(), t.max())


def verdict(a_name, a, b_name, b):
    a, b = np.asarray(a), np.asarray(b)
    ratio = np.median(b) / np.median(a)
    if a.max() < b.min():
        return "%s is faster than %s: its maximum lies below the other's minimum; ratio of medians %.2f" % (a_name, b_name, ratio)
    if b.max() < a.min():
        return "%s is faster than %s: its maximum lies below the other's minimum; ratio of medians %.2f" % (b_name, a_name, 1 / ratio)
    return "neither %s nor %s is faster: their ranges overlap; ratio of medians (%s / %s) %.2f" % (a_name, b_name, b_name, a_name, ratio)


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "sphere_inputs_bench.txt")
    rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    warmup = 3
    scenes = [make_scene(s) for s in range(S)]
    pots = [np.random.default_rng(100 + s).random(NPOT) * 1e-3 for s in range(S)]
    ss = si.SphereScenes(scenes, R_IN, MARGIN, init_potentials=[p.copy() for p in pots])
    sampler = picking.PotentialSphereSampler([s["pot_points"] for s in scenes], [s["points"] for s in scenes], R_IN, MARGIN,
                                             init_potentials=[p.copy() for p in pots])
    noise = (torch.randn((CAP, 3), device=dev) * Cfg.augment_noise).contiguous()

    def draws_for(round_):
        np.random.seed(round_)
        return si.draw_spheres(Cfg, B, NV, FLIP)

    # round 0 of both paths from the same potentials and draws: the same spheres, the same bits
    d0 = draws_for(0)
    got = si.sphere_batch(ss, Cfg, B, 1 << 40, CAP, NV, k=K, noise=noise, draws=d0)
    want = parent_batch(scenes, sampler, d0, noise)
    total = int(got["q_off"][-1].item())
    lens = got["stack_lengths"].cpu().numpy()
    same = all(torch.equal(got[key][:total], w) for key, w in zip(("points", "features", "labels", "input_inds",
                                                                    "feat_aggre_points", "knn", "knn_stacked"), want[:7]))
    same &= torch.equal(got["images"], want[7]) and torch.equal(got["image_xyz"], want[8]) and torch.equal(got["image_mask"], want[9])
    status = got["status"].cpu().numpy().tolist()

    dev_ev, dev_wall, par_ev, par_wall, stage_ms = [], [], [], [], {s: [] for s in STAGES}
    rag_ev, calls_ev = [], []
    knn_equal = True
    for it in range(1, 1 + warmup + rounds):
        draws = draws_for(it)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        e0.record()
        si.sphere_batch(ss, Cfg, B, 1 << 40, CAP, NV, k=K, noise=noise, draws=draws)
        e1.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        p0, p1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t2 = time.perf_counter()
        p0.record()
        parent_batch(scenes, sampler, draws, noise)
        p1.record()
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        events = [torch.cuda.Event(enable_timing=True) for _ in range(9)]
        rows, q_off, keys, image_mask, knn = staged_device_batch(ss, draws, noise, events)
        sampler.pick(), sampler.pick(), sampler.pick(), sampler.pick(), sampler.pick()      # keep the two potentials in step
        torch.cuda.synchronize()
        # comparison 2 on this batch's items; the lengths are handed to the host for free
        q = q_off.cpu().numpy()
        points = ss.resident.points
        queries = [points[rows[q[b]:q[b + 1]]].contiguous() for b in range(B)]
        torch.cuda.synchronize()
        r0, r1, c0, c1 = (torch.cuda.Event(enable_timing=True) for _ in range(4))
        r0.record()
        ragged = ops.knn_f64_ragged(points, rows, q_off, keys, image_mask, k=K)
        r1.record()
        c0.record()
        alone = [ops.knn_pixels(queries[b], keys[b], image_mask[b], k=K) for b in range(B)]
        c1.record()
        torch.cuda.synchronize()
        knn_equal &= torch.equal(ragged[:q[-1]], torch.cat(alone))
        if it > warmup:
            dev_ev.append(e0.elapsed_time(e1)), dev_wall.append(1e3 * (t1 - t0))
            par_ev.append(p0.elapsed_time(p1)), par_wall.append(1e3 * (t3 - t2))
            for i, s in enumerate(STAGES):
                stage_ms[s].append(events[i].elapsed_time(events[i + 1]))
            rag_ev.append(r0.elapsed_time(r1)), calls_ev.append(c0.elapsed_time(c1))

    lines = ["sphere_inputs_bench: B = %d spheres of in_radius %.1f from %d scenes of %d points, %d potential points, %d frames "
             "of %d x %d and %d base points each; %d views and %d neighbours per sphere, flip %.1f, noise; sphere sizes in round "
             "0: %s, status %s. median [min .. max] ms over %d rounds after %d warm-ups, paths alternating. Round 0 of the device "
             "batch bit-equal to the parent path's from the same potentials and draws: %s"
             % (B, R_IN, S, N, NPOT, NF, H, W, NB, NV, K, FLIP, lens.tolist(), status, rounds, warmup, same),
             "1. a batch", "  device  sphere_batch                 wall clock %s   HIP events %s" % (fmt(dev_wall), fmt(dev_ev))]
    lines += ["            %-22s HIP events %s" % (s, fmt(stage_ms[s])) for s in STAGES]
    lines += ["  parent  pick() / isin + select_frames / unproject_depth / knn_pixels / torch, one sphere at a time",
              "                                       wall clock %s   HIP events %s" % (fmt(par_wall), fmt(par_ev)),
              "  " + verdict("device", dev_wall, "parent", par_wall) + " (wall clock)",
              "2. the k-NN of one batch's items (%d views of %d x %d pixels as keys per item), results equal in every round: %s"
              % (NV, H, W, knn_equal),
              "  ragged  mvk_knn_f64_ragged, one call             HIP events %s" % fmt(rag_ev),
              "  B calls mvk_knn_f64 per item, lengths for free   HIP events %s" % fmt(calls_ev),
              "  " + verdict("ragged", rag_ev, "B calls", calls_ev) + " (HIP events)",
              "not measured: real ScanNet scenes, an epoch end to end"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
