"""The whole-scene test of the MVPNet baseline with several chunks per forward (not in the reference).

``mvpnet.test_mvpnet_3d.predict_whole_scene`` forwards a scene's chunks one at a time. Here G chunks of different sizes
go through the network in one call, as a zero-padded batch with the chunks' sizes in data_batch['lengths'], which
PN2SSG hands to farthest point sampling and the ball query of its first set abstraction: each chunk gets the centroids
and neighbours it gets alone.

* ``collate_chunks``               several chunks' tensors as one padded batch with 'lengths'
* ``chunk_groups``                 the chunks of an iterable G at a time, sparse chunks padded the reference's way
* ``predict_whole_scene_grouped``  the loop; with chunks_per_forward = 1 it is ``predict_whole_scene`` itself
* ``vote_groups``                  the model / vote loop over such groups, shared with mvpnet/whole_scene_inputs.py

``test_mvpnet_3d.py`` carries a test file's name and stays as it is, so the loop is a function of its own here and not
a keyword of ``predict_whole_scene``; the padding of a sparse chunk and the scaffold around the loop are restated
(``_pad_sparse_chunk``). tests/test_pn2_ragged_{cpu,gpu}.py hold the two copies together: same pad draws, and G > 1
bit-equal to G = 1 on a scene with a sparse chunk."""
import numpy as np
import torch
import torch.nn.functional as F

try:
    from .test_mvpnet_3d import WholeSceneVoter, predict_whole_scene
except ImportError:  # dropin/ put on sys.path directly
    from mvpnet.test_mvpnet_3d import WholeSceneVoter, predict_whole_scene

_POINT_DIM = {'points': 1, 'knn_indices': 0}          # the keys that are sized by the chunk, and where


def _pad_sparse_chunk(data_dict, min_nb_pts, device):
    """A chunk's tensors (all keys but 'chunk_ind') on `device`; a chunk of fewer than min_nb_pts points is padded as
    predict_whole_scene pads it (reference test_mvpnet_3d.py:153-158): the same draw from the global NumPy generator."""
    data_dict = {k: torch.as_tensor(v).to(device) for k, v in data_dict.items() if k != 'chunk_ind'}
    nc = data_dict['points'].shape[1]                               # points are (3, nc)
    if nc < min_nb_pts:
        extra = np.random.randint(nc, size=min_nb_pts - nc)
        rows = torch.from_numpy(np.concatenate([np.arange(nc), extra])).to(device)
        data_dict['points'] = data_dict['points'].index_select(1, rows)
        data_dict['knn_indices'] = data_dict['knn_indices'].index_select(0, rows)
    return data_dict


def _group_shape(data_dict):
    """What the chunks of one forward must share: every key's shape, the point dimension left out."""
    return {k: tuple(s for d, s in enumerate(v.shape) if d != _POINT_DIM.get(k, -1)) for k, v in data_dict.items()}


def collate_chunks(dicts):
    """One batch from the tensors of several chunks (dicts without 'chunk_ind', on one device, host or HBM): 'points'
    (3, n_g) -> (G, 3, n_max) and 'knn_indices' (n_g, k) -> (G, n_max, k), zero-padded behind each chunk's own rows
    (pixel 0 is a valid index); every other key stacked as it is, so its shape must be the same in all chunks;
    'lengths' (G,) int64 = n_g on the points' device. ValueError when the chunks do not fit one batch."""
    if not dicts:
        raise ValueError("collate_chunks: no chunk")
    if any(_group_shape(d) != _group_shape(dicts[0]) for d in dicts[1:]):
        raise ValueError("collate_chunks: the chunks differ in more than their point counts")
    sizes = [d['points'].shape[1] for d in dicts]
    n_max = max(sizes)
    batch = {}
    for k, v in dicts[0].items():
        if k in _POINT_DIM:     # F.pad counts dimensions from the last: zeros behind the point dimension only
            lead = [0, 0] * (v.dim() - 1 - _POINT_DIM[k])
            batch[k] = torch.stack([F.pad(d[k], lead + [0, n_max - n]) for d, n in zip(dicts, sizes)])
        else:
            batch[k] = torch.stack([d[k] for d in dicts])
    batch['lengths'] = torch.tensor(sizes, dtype=torch.int64, device=dicts[0]['points'].device)
    return batch


def chunk_groups(chunk_inputs, chunks_per_forward, min_nb_pts, device):
    """The chunks of an iterable, in order, as (batch, [chunk_ind, ...]) with up to chunks_per_forward chunks per batch
    (``collate_chunks``). Sparse chunks are padded one by one in the iterable's order, so the draws from the global
    NumPy generator are those of the one-chunk loop. A group closes early at a chunk whose tensors differ from the
    group's in more than the point count (images, image_xyz, the k of knn_indices); that chunk opens the next group."""
    group, inds = [], []
    for data_dict in chunk_inputs:
        chunk_ind = data_dict['chunk_ind']
        data_dict = _pad_sparse_chunk(data_dict, min_nb_pts, device)
        if group and (len(group) == chunks_per_forward or _group_shape(data_dict) != _group_shape(group[0])):
            yield collate_chunks(group), inds
            group, inds = [], []
        group.append(data_dict)
        inds.append(chunk_ind)
    if group:
        yield collate_chunks(group), inds


def predict_whole_scene_grouped(model, points, chunk_inputs, min_nb_pts=2048, seg_label=None, evaluator=None,
                                num_classes=None, chunks_per_forward=1):
    """``predict_whole_scene`` with its arguments and results, forwarding chunks_per_forward = G chunks per call of the
    model, which must take data_batch['lengths'] as PN2SSG and MVPNet3D do (inference only). The chunks are taken G at
    a time in order, zero-padded to the group's largest and stacked (``chunk_groups``, ``collate_chunks``); sparse chunks
    are padded exactly as with G = 1; the logit columns behind a chunk's own are unspecified and do not vote. The chunks
    vote one by one in the iterable's order, so the float32 sums keep the reference's order. G = 1 calls
    ``predict_whole_scene``."""
    chunks_per_forward = int(chunks_per_forward)
    if chunks_per_forward < 1:
        raise ValueError("predict_whole_scene_grouped: chunks_per_forward must be >= 1")
    if chunks_per_forward == 1:
        return predict_whole_scene(model, points, chunk_inputs, min_nb_pts=min_nb_pts, seg_label=seg_label,
                                   evaluator=evaluator, num_classes=num_classes)
    return vote_groups(model, points, chunk_groups(chunk_inputs, chunks_per_forward, min_nb_pts, points.device),
                       seg_label=seg_label, evaluator=evaluator, num_classes=num_classes,
                       who="predict_whole_scene_grouped")


def vote_groups(model, points, groups, seg_label=None, evaluator=None, num_classes=None, who="vote_groups"):
    """The model / vote loop of ``predict_whole_scene_grouped`` over an iterable of (data_batch, [chunk_ind, ...]) as
    ``chunk_groups`` yields them: under model.eval() and torch.no_grad() every batch is forwarded once and its chunks
    vote one by one in order, then the scene is finished (and scored, with seg_label and an evaluator). An exception
    that the iterable raises leaves the model in its mode and the evaluator untouched. Returns (pred_label, mean_logit)
    in HBM."""
    device = points.device
    num_points = len(points)
    if num_classes is None and evaluator is not None:
        num_classes = evaluator.num_classes
    voter = None
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            for data_batch, chunk_inds in groups:
                seg_logit = model(data_batch)['seg_logit']                      # (G, num_classes, n_max)
                if voter is None:
                    voter = WholeSceneVoter(num_points, seg_logit.shape[1] if num_classes is None else num_classes, device)
                for g, chunk_ind in enumerate(chunk_inds):
                    voter.add(seg_logit[g], chunk_ind)
    finally:
        model.train(was_training)
    if voter is None:
        if num_classes is None:
            raise ValueError("%s: a scene without chunks needs num_classes or an evaluator" % who)
        voter = WholeSceneVoter(num_points, num_classes, device)
    return voter.finish(seg_label, evaluator)
