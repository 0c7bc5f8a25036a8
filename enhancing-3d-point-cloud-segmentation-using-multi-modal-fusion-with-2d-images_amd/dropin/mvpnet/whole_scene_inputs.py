"""The inputs of the MVPNet whole-scene test built on the device, G chunks at a time (not in the reference).

``mvpnet.test_mvpnet_3d.chunk_rgbd_inputs`` makes one chunk's inputs with about fifteen tensor operations and seven k-NN
launches, and waits for the device num_rgbd_frames + 1 times (one argmax per chosen frame, the count of valid pixels);
``whole_scene_grouped.collate_chunks`` then pads and stacks G of them. Here a group of G chunks goes from the scene, the
scan's frames and the chunks' index rows in HBM to the padded batch in a fixed handful of launches (csrc/scene_inputs.hip)
with nothing read back:

* ``SceneFrames``              a scan's frames with what is made once per scene: the overlap table as bit rows, the
                               inverse intrinsics, the depth as 16-bit words
* ``group_rgbd_inputs``        the generator of (data_batch, chunk_inds): what ``chunk_groups`` yields over
                               ``chunk_rgbd_inputs`` of every chunk, bit for bit, plus 'num_valid_pixels'
* ``predict_whole_scene_rgbd`` ``predict_whole_scene_grouped`` fed by it

``test_mvpnet_3d.py`` and ``whole_scene_grouped.py`` keep their functions; this is a separate, opt-in entry point."""
import numpy as np
import torch

try:
    from .._native import ops
    from .whole_scene_grouped import vote_groups
except ImportError:  # dropin/ put on sys.path directly
    from _native import ops
    from mvpnet.whole_scene_grouped import vote_groups

PIXEL_MARGIN = 0.1           # get_rgbd_data widens the chunk's xy box by this much for the pixels (scannet_2d3d.py:255-281)


def _in_hbm(name, t):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError("whole_scene_inputs: %s must be a tensor resident in HBM; there is no CPU fallback" % name)
    return t


class SceneFrames(object):
    """All frames of one scan, as ``chunk_rgbd_inputs`` takes them -- 'depth' (nf, h, w) integer millimetres, 'images'
    (nf, h, w, 3) already normalised, 'poses' (nf, 4, 4), 'base_point_ind' (nb,), 'pointwise_rgbd_overlap' (nb, nf) in
    HBM and 'cam_matrix' on the host, already rescaled to (h, w) -- and what every chunk of the scene shares: the overlap
    table as frame-major bit rows (``ops.overlap_pack``), the inverse intrinsics computed as ``ops.unproject_depth``
    computes them, the depth as int16 words and float32 images and poses."""

    def __init__(self, frames):
        self.frames = frames
        depth = _in_hbm("frames['depth']", frames['depth'])
        self.depth16 = (depth if depth.dtype == torch.int16 else depth.to(torch.int16)).contiguous()
        self.num_frames, self.h, self.w = self.depth16.shape
        self.images = _in_hbm("frames['images']", frames['images']).float().contiguous()
        self.poses = _in_hbm("frames['poses']", frames['poses']).float().contiguous()
        self.base_point_ind = _in_hbm("frames['base_point_ind']", frames['base_point_ind']).to(torch.int64).contiguous()
        overlap = _in_hbm("frames['pointwise_rgbd_overlap']", frames['pointwise_rgbd_overlap'])
        if overlap.dtype not in (torch.bool, torch.uint8):
            overlap = overlap.bool()
        if overlap.dim() != 2 or tuple(overlap.shape) != (self.base_point_ind.shape[0], self.num_frames):
            raise ValueError("SceneFrames: pointwise_rgbd_overlap must be (len(base_point_ind), number of frames)")
        self.num_base = overlap.shape[0]
        self.overlap_bits = ops.overlap_pack(overlap)
        cam = np.asarray(frames['cam_matrix'], dtype=np.float32)[:3, :3]
        self.cam_inv = np.ascontiguousarray(np.linalg.inv(cam).astype(np.float64))      # a float32 inverse, as ops.unproject_depth


def _chunk_rows(chunk_indices, device):
    """The chunks' index vectors as one int64 buffer in HBM and each chunk's offset in it. The views of one CSR buffer
    that ``scene2chunks_legacy`` returns are used where they lie; anything else is concatenated (one copy per scene)."""
    if not chunk_indices:
        return torch.zeros((0,), dtype=torch.int64, device=device), []
    first = chunk_indices[0]
    if all(isinstance(i, torch.Tensor) and i.device == device and i.dtype == torch.int64 and i.dim() == 1 and
           i.is_contiguous() and i.untyped_storage().data_ptr() == first.untyped_storage().data_ptr()
           for i in chunk_indices):
        storage = first.untyped_storage()
        rows = torch.empty((0,), dtype=torch.int64, device=device).set_(storage, 0, (storage.nbytes() // 8,))
        return rows, [int(i.storage_offset()) for i in chunk_indices]
    parts = [torch.as_tensor(i).to(device=device, dtype=torch.int64).reshape(-1) for i in chunk_indices]
    return torch.cat(parts), np.concatenate([[0], np.cumsum([len(p) for p in parts])])[:-1].tolist()


def _upload(words, device):
    """A host int64 array to HBM through pinned memory, without a wait."""
    staged = torch.empty((len(words),), dtype=torch.int64, pin_memory=True)
    staged.numpy()[:] = words
    return staged.to(device, non_blocking=True)


def group_rgbd_inputs(points, chunk_indices, chunk_boxes, scene_frames, num_rgbd_frames, k=3, chunks_per_forward=1,
                      min_nb_pts=2048):
    """Generator of (data_batch, chunk_inds), G = chunks_per_forward chunks at a time: exactly what
    ``chunk_groups((chunk_rgbd_inputs(points, ind, box, frames, num_rgbd_frames, k) for every chunk), G, min_nb_pts,
    device)`` yields -- 'points' (G, 3, n_max), 'images' (G, nv, 3, h, w), 'image_xyz' (G, nv, h, w, 3), 'image_mask'
    (G, nv, h, w), 'knn_indices' (G, n_max, k), 'lengths' (G,) int64, the same bits -- plus 'num_valid_pixels' (G,) int32.

    points (num_points, 3) float32 in HBM; chunk_indices / chunk_boxes as ``scene2chunks_legacy(..., return_bbox=True)``
    returns them: every index vector ASCENDING and DISTINCT (the frame choice finds a chunk's base points by binary
    search in it); scene_frames: a ``SceneFrames``. A chunk below min_nb_pts is padded with the same draws from the global
    NumPy generator, in chunk order, as ``predict_whole_scene`` makes (the chunk sizes are known on the host). A group
    costs one small upload from pinned memory and six launches besides the k-NN's own; nothing is read back and nothing
    waits for the device.

    One difference: ``chunk_rgbd_inputs`` raises ValueError at a chunk with fewer than k valid pixels. Here that chunk's
    'knn_indices' are -1 where no neighbour exists and 'num_valid_pixels' says so; the caller decides when to look
    (``predict_whole_scene_rgbd`` looks once per scene)."""
    G, nv, k = int(chunks_per_forward), int(num_rgbd_frames), int(k)
    if G < 1:
        raise ValueError("group_rgbd_inputs: chunks_per_forward must be >= 1")
    if len(chunk_indices) != len(chunk_boxes):
        raise ValueError("group_rgbd_inputs: one box per chunk expected")
    _in_hbm("points", points)
    if points.dtype != torch.float32 or points.dim() != 2 or points.shape[1] != 3:
        raise RuntimeError("group_rgbd_inputs: points must be a float32 (num_points, 3) tensor")
    sf, device = scene_frames, points.device
    pts = points.contiguous()
    rows, offsets = _chunk_rows(chunk_indices, device)
    sizes = [len(i) for i in chunk_indices]
    for start in range(0, len(sizes), G):
        stop = min(start + G, len(sizes))
        n = stop - start
        row_len = np.asarray(sizes[start:stop], np.int64)
        extras = [np.random.randint(nc, size=min_nb_pts - nc).astype(np.int32) if nc < min_nb_pts else np.zeros(0, np.int32)
                  for nc in row_len.tolist()]
        lengths = row_len + np.asarray([len(e) for e in extras], np.int64)
        bounds = np.empty((n, 4), np.float64)
        for g in range(n):
            box = np.asarray(chunk_boxes[start + g], dtype=np.float64)[[0, 1, 3, 4]]
            bounds[g] = (float(box[0] - PIXEL_MARGIN), float(box[2] + PIXEL_MARGIN),
                         float(box[1] - PIXEL_MARGIN), float(box[3] + PIXEL_MARGIN))
        extra = np.concatenate(extras + [np.zeros(1, np.int32)])
        extra = np.concatenate([extra, np.zeros(len(extra) % 2, np.int32)])
        # one upload: row_off | row_len | lengths | q_off | extra_off | bounds as words | extras as words
        words = np.concatenate([np.asarray(offsets[start:stop], np.int64), row_len, lengths,
                                np.concatenate([[0], np.cumsum(row_len)]).astype(np.int64),
                                np.concatenate([[0], np.cumsum([len(e) for e in extras])]).astype(np.int64),
                                bounds.reshape(-1).view(np.int64), extra.view(np.int64)])
        meta = _upload(words, device)
        row_off_d, row_len_d, lengths_d = meta[0:n], meta[n:2 * n], meta[2 * n:3 * n]
        q_off_d, extra_off_d = meta[3 * n:4 * n + 1], meta[4 * n + 1:5 * n + 2]
        bounds_d = meta[5 * n + 2:9 * n + 2].view(torch.float64).view(n, 4)
        extras_d = meta[9 * n + 2:].view(torch.int32)

        sel = ops.chunk_select_frames(sf.overlap_bits, sf.num_base, sf.base_point_ind, rows, row_off_d, row_len_d, nv)
        keys, image_xyz, image_mask, images, num_valid = ops.chunk_unproject(sel, sf.depth16, sf.images, sf.poses,
                                                                             sf.cam_inv, bounds_d)
        queries, knn = ops.chunk_knn_many(pts, rows, row_off_d, q_off_d, row_len, keys, image_mask, k=k)
        batch_points, batch_knn = ops.chunk_batch_rows(queries, knn, q_off_d, row_len_d, lengths_d, extras_d, extra_off_d,
                                                       int(lengths.max()))
        data_batch = {'points': batch_points, 'images': images, 'image_xyz': image_xyz, 'image_mask': image_mask,
                      'knn_indices': batch_knn, 'lengths': lengths_d, 'num_valid_pixels': num_valid}
        yield data_batch, [rows[offsets[i]:offsets[i] + sizes[i]] for i in range(start, stop)]


def predict_whole_scene_rgbd(model, points, chunk_indices, chunk_boxes, scene_frames, num_rgbd_frames, k=3,
                             min_nb_pts=2048, seg_label=None, evaluator=None, num_classes=None, chunks_per_forward=1):
    """One scene of the whole-scene test from the scene, its chunks and its frames: the results of
    ``predict_whole_scene_grouped(model, points, [chunk_rgbd_inputs(...) for every chunk], ...)`` on the same chunks, with
    the inputs built by ``group_rgbd_inputs``. The model must take data_batch['lengths'] (PN2SSG, MVPNet3D), also at
    chunks_per_forward = 1. Returns pred_label [num_points] int64 and mean_logit [num_points, num_classes] float32 in HBM.

    The counts of valid pixels are read ONCE per scene, after the last group. If a chunk had fewer than k, ValueError is
    raised with scikit-learn's message as ``chunk_rgbd_inputs`` words it, naming the first such chunk -- at the END of the
    scene, not at the chunk: the earlier chunks have been forwarded by then, the scene is not finished and the evaluator
    is not updated. The -1 neighbours of such a chunk reach the model as pixel 0."""
    counts = []

    def groups():
        for data_batch, chunk_inds in group_rgbd_inputs(points, chunk_indices, chunk_boxes, scene_frames, num_rgbd_frames,
                                                        k=k, chunks_per_forward=chunks_per_forward, min_nb_pts=min_nb_pts):
            counts.append(data_batch['num_valid_pixels'])
            data_batch['knn_indices'].clamp_(min=0)          # only a chunk that fails below has an entry to clamp
            yield data_batch, chunk_inds
        if counts:
            for chunk, n_valid in enumerate(torch.cat(counts).cpu().tolist()):
                if n_valid < k:
                    raise ValueError("Expected n_neighbors <= n_samples,  but n_samples = %d, n_neighbors = %d (chunk %d)"
                                     % (n_valid, k, chunk))

    return vote_groups(model, points, groups(), seg_label=seg_label, evaluator=evaluator, num_classes=num_classes,
                       who="predict_whole_scene_rgbd")
