"""The whole-scene test of the MVPNet baseline (reference mvpnet/test_mvpnet_3d.py:126-233) with the scene resident in
HBM: the chunk loop, the per-point logit votes and the score.

* ``WholeSceneVoter``      the arrays pred_logit_whole_scene / num_pred_per_point of :141-142 in HBM and the lines
                           :164-178 on them (csrc/chunk.hip): chunks vote in call order, so the float32 sums are the
                           reference's bit for bit; the visit counter is int32, not uint8.
* ``predict_whole_scene``  the loop of :141-194 under model.eval() and torch.no_grad(), sparse chunks padded the
                           reference's way (:153-158).
* ``chunk_rgbd_inputs``    the arithmetic of ScanNet2D3DChunks.get_rgbd_data (mvpnet/data/scannet_2d3d.py:199-321) for
                           frames that are already in HBM.

Out of scope here: argument parsing, the configuration and checkpointer, the dataset's files (loading, resizing, colour
jitter, flips), the open3d debug output and the submission files of :203-207."""
import numpy as np
import torch

try:
    from .._native import ops
    from ..utils.voting import select_frames
except ImportError:  # dropin/ put on sys.path directly
    from _native import ops
    from utils.voting import select_frames


class WholeSceneVoter(object):
    """Logit sums [num_points, num_classes] float32 and visit counts [num_points] int32 of one scene, in HBM."""

    def __init__(self, num_points, num_classes, device):
        self.num_points, self.num_classes = int(num_points), int(num_classes)
        self.logit_sum = torch.zeros((self.num_points, self.num_classes), dtype=torch.float32, device=device)
        self.num_pred = torch.zeros((self.num_points,), dtype=torch.int32, device=device)

    def add(self, seg_logit, chunk_ind):
        """seg_logit (num_classes, >= len(chunk_ind)) as the network returns it (a leading batch dimension of 1 is
        dropped); only the first len(chunk_ind) columns vote (:164-168). chunk_ind: int64, distinct."""
        if seg_logit.dim() == 3:
            seg_logit = seg_logit.squeeze(0)
        chunk_ind = torch.as_tensor(chunk_ind).to(device=self.logit_sum.device, dtype=torch.int64)
        ops.chunk_vote_add(self.logit_sum, self.num_pred, seg_logit, chunk_ind)

    def finish(self, seg_label=None, evaluator=None):
        """pred_label [num_points] int64 and mean_logit [num_points, num_classes] float32 (:171-178): the mean over
        the visits, its first maximum, num_classes where a point was never visited. The mean overwrites the sums: a
        voter is finished once. With seg_label and an evaluator the scene is scored (:192-193) and only the
        [num_classes, num_classes] counts go to the host."""
        if seg_label is None or evaluator is None:
            return ops.chunk_vote_finish(self.logit_sum, self.num_pred, in_place=True)
        seg_label = torch.as_tensor(seg_label).to(self.logit_sum.device)
        if evaluator.num_classes == self.num_classes and np.array_equal(evaluator.labels, np.arange(self.num_classes)):
            pred, mean, conf = ops.chunk_vote_finish(self.logit_sum, self.num_pred, labels=seg_label, in_place=True)
            evaluator.confusion_matrix += conf.cpu().numpy()
        else:
            pred, mean = ops.chunk_vote_finish(self.logit_sum, self.num_pred, in_place=True)
            evaluator.update(pred, seg_label)
        return pred, mean


def predict_whole_scene(model, points, chunk_inputs, min_nb_pts=2048, seg_label=None, evaluator=None, num_classes=None):
    """One scene of the reference's test loop (:141-194). points: the scene's (num_points, 3) tensor in HBM (its length
    and device are used). chunk_inputs: an iterable of dicts with 'points' (3, nc), 'chunk_ind' (nc,), 'images',
    'image_xyz' and 'knn_indices' (nc, k), as ``chunk_rgbd_inputs`` makes them. A chunk with fewer than min_nb_pts
    points is padded as in :153-158: the pad is drawn on the host from the global NumPy generator, the rows of 'points'
    and 'knn_indices' are gathered on the device, and only the first len(chunk_ind) logit columns vote. Between chunks
    nothing sized by the chunk goes to the host. num_classes is needed only for a scene without chunks and no
    evaluator. Returns pred_label [num_points] int64 and mean_logit [num_points, num_classes] float32, both in HBM."""
    device = points.device
    num_points = len(points)
    if num_classes is None and evaluator is not None:
        num_classes = evaluator.num_classes
    voter = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for data_dict in chunk_inputs:
                chunk_ind = data_dict['chunk_ind']
                data_dict = {k: torch.as_tensor(v).to(device) for k, v in data_dict.items() if k != 'chunk_ind'}
                nc = data_dict['points'].shape[1]                               # points are (3, nc)
                if nc < min_nb_pts:
                    # repeat randomly drawn points behind the chunk's own: the same draw from the global generator
                    # as the reference's, so a seeded run pads with the same points
                    extra = np.random.randint(nc, size=min_nb_pts - nc)
                    rows = torch.from_numpy(np.concatenate([np.arange(nc), extra])).to(device)
                    data_dict['points'] = data_dict['points'].index_select(1, rows)
                    data_dict['knn_indices'] = data_dict['knn_indices'].index_select(0, rows)
                data_batch = {k: v.unsqueeze(0) for k, v in data_dict.items()}
                seg_logit = model(data_batch)['seg_logit'].squeeze(0)
                if voter is None:
                    voter = WholeSceneVoter(num_points, seg_logit.shape[0] if num_classes is None else num_classes, device)
                voter.add(seg_logit, chunk_ind)
    finally:
        model.train(was_training)
    if voter is None:
        if num_classes is None:
            raise ValueError("predict_whole_scene: a scene without chunks needs num_classes or an evaluator")
        voter = WholeSceneVoter(num_points, num_classes, device)
    return voter.finish(seg_label, evaluator)


def chunk_rgbd_inputs(points, chunk_ind, chunk_box, frames, num_rgbd_frames, k=3):
    """The network inputs of one chunk (get_rgbd_data, scannet_2d3d.py:199-321, and :532-562) from a scene in HBM.

    points (num_points, 3) float32 and chunk_ind (nc,) int64 in HBM; chunk_box: the chunk's (x1, y1, z1, x2, y2, z2) as
    ``scene2chunks_legacy`` returns it. frames, all frames of the scan: 'depth' (nf, h, w) integer millimetres, 'images'
    (nf, h, w, 3) float32 already normalised, 'poses' (nf, 4, 4) float32, 'base_point_ind' (nb,) int64,
    'pointwise_rgbd_overlap' (nb, nf) bool -- in HBM -- and 'cam_matrix', a host array already rescaled to (h, w).
    Frames: greedy maximum coverage of the chunk's base points (:199-221). Pixels: unprojected in float64, valid where
    the depth is positive and strictly inside the chunk's xy box widened by 0.1, compared in float64 (:255-281). k-NN:
    exact, among the valid pixels of the chosen frames, as flat pixel indices (:298-313). Returns the dict that
    ``predict_whole_scene`` takes, 'image_xyz' as float32 and 'image_mask' besides. Fewer than k valid pixels raise
    ValueError, as scikit-learn's kneighbors does."""
    num_points = points.shape[0]
    chunk_ind = chunk_ind.to(torch.int64)
    chunk_mask = torch.zeros((num_points,), dtype=torch.bool, device=points.device)
    chunk_mask[chunk_ind] = True
    in_chunk = chunk_mask[frames['base_point_ind'].to(torch.int64)]                       # (nb,)
    selected = select_frames(frames['pointwise_rgbd_overlap'].bool()[in_chunk], num_rgbd_frames)
    sel = torch.as_tensor(selected, dtype=torch.int64, device=points.device)
    images = frames['images'].index_select(0, sel)                                        # (nv, h, w, 3)
    image_xyz, image_mask = ops.unproject_depth(frames['depth'].index_select(0, sel), frames['cam_matrix'],
                                                frames['poses'].index_select(0, sel))     # float64, depth > 0
    box = np.asarray(chunk_box, dtype=np.float64)[[0, 1, 3, 4]]
    pixel_margin = 0.1
    x, y = image_xyz[..., 0], image_xyz[..., 1]
    image_mask = (image_mask & (x > float(box[0] - pixel_margin)) & (x < float(box[2] + pixel_margin)) &
                  (y > float(box[1] - pixel_margin)) & (y < float(box[3] + pixel_margin)))
    n_valid = int(image_mask.sum())
    if n_valid < k:
        raise ValueError("Expected n_neighbors <= n_samples,  but n_samples = %d, n_neighbors = %d" % (n_valid, k))
    chunk_points = points.index_select(0, chunk_ind)                                      # (nc, 3)
    knn_indices = ops.knn_pixels(chunk_points, image_xyz, image_mask, k=k)
    return {
        'points': chunk_points.t().contiguous(),                                          # (3, nc)
        'chunk_ind': chunk_ind,
        'images': images.permute(0, 3, 1, 2).contiguous().float(),                        # (nv, 3, h, w)
        'image_xyz': image_xyz.float(),                                                   # (nv, h, w, 3)
        'image_mask': image_mask,                                                         # (nv, h, w)
        'knn_indices': knn_indices,                                                       # (nc, k)
    }
