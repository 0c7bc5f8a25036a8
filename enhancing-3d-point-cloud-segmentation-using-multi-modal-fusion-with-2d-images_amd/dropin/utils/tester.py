"""utils.tester of the reference under its own names (KPConv-PyTorch/utils/tester.py:79-376
ModelTester.cloud_segmentation_test) plus the validation loop of its trainer (utils/trainer.py:283-535) as a function,
with the votes resident in HBM.

The reference copies every batch's probabilities and points to the host, loops over the spheres in Python with NumPy
fancy indexing into float64 per-cloud arrays, and later runs np.insert / argmax / confusion_matrix over whole clouds.
Here the network runs frozen (models.blocks.freeze_inference) under torch.no_grad(), the float64 votes of all clouds
live in one device buffer (VoteAccumulator) and three kernels (csrc/vote.hip) do the softmax + vote, the widened
argmax + reprojection and the confusions. Per batch only the B cloud indices come to the host; at the reference's
checkpoints the [Ctot, Ctot] confusions and -- when config.saving -- the predictions that are written to disk.

Left out: the open3d colour files (`*_visualize.ply`, tester.py:341-342; open3d is not a dependency here) and the
potentials files (tester.py:354-360: they need the dataset's KD-trees, which the drop-in datasets do not build).
"""
import time
from os import makedirs
from os.path import exists, join

import numpy as np
import torch

try:
    from .._native import ops
    from ..models.blocks import freeze_inference
    from .metrics import IoU_from_confusions
    from .ply import write_ply
except ImportError:  # dropin/ put on sys.path directly
    from _native import ops
    from models.blocks import freeze_inference
    from utils.metrics import IoU_from_confusions
    from utils.ply import write_ply


class VoteAccumulator:
    """The float64 votes of a set of clouds in HBM (the reference's `self.test_probs` / `self.validation_probs`,
    tester.py:100, trainer.py:313): one [sum of cloud sizes, num_model_classes] buffer with a row-offset table.

    label_values: the dataset's full label table (sorted raw values, ignored ones included); ignored_labels: the values
    the model has no column for. The column map built from them says where the reference np.inserts a zero column."""

    def __init__(self, cloud_sizes, num_model_classes, label_values, ignored_labels, device, smooth=0.95):
        self.device = torch.device(device)
        self.smooth = float(smooth)
        self.C = int(num_model_classes)
        sizes = [int(n) for n in cloud_sizes]
        self.offsets_host = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.offsets = torch.from_numpy(self.offsets_host).to(self.device)
        self.votes = torch.zeros((int(self.offsets_host[-1]), self.C), dtype=torch.float64, device=self.device)
        self.label_values_host = np.asarray(label_values).astype(np.int32).reshape(-1)
        ignored = set(int(v) for v in ignored_labels)
        col_map, col = [], 0
        for v in self.label_values_host:
            if int(v) in ignored:
                col_map.append(-1)
            else:
                col_map.append(col)
                col += 1
        if col != self.C:
            raise ValueError('{:d} labels are not ignored but the model predicts {:d} classes'.format(col, self.C))
        self.col_map_host = np.asarray(col_map, np.int32)
        self.kept = self.col_map_host >= 0                  # rows / columns np.delete leaves (tester.py:242-245)
        self.label_values = torch.from_numpy(self.label_values_host).to(self.device)
        self.col_map = torch.from_numpy(self.col_map_host).to(self.device)
        self.Ctot = len(col_map)
        self._confusion = torch.zeros((self.Ctot, self.Ctot), dtype=torch.int64, device=self.device)

    @property
    def num_clouds(self):
        return len(self.offsets_host) - 1

    def update(self, batch, outputs, radius_ratio=None, in_radius=None, labels=None, is_logits=True):
        """One batch's votes (tester.py:160-186 with radius_ratio / in_radius, trainer.py:351-378 without). outputs
        [N, C]: the network's logits (is_logits=False: probabilities). labels [N] (the batch's own, trainer.py:352):
        this batch's argmax is also counted into confusion(). Returns the B cloud indices (host), the only thing read
        back."""
        r2_max = 0.0
        points = None
        if radius_ratio is not None and 0 < radius_ratio < 1:
            r2_max = (radius_ratio * in_radius) ** 2
            points = batch.points[0]
        cloud_inds = batch.cloud_inds
        host = cloud_inds.cpu().numpy() if isinstance(cloud_inds, torch.Tensor) else np.asarray(cloud_inds)
        host = np.ascontiguousarray(host.reshape(-1), dtype=np.int32)
        if host.size and (host.min() < 0 or host.max() >= self.num_clouds):
            raise ValueError('cloud_inds outside the {:d} clouds of this accumulator'.format(self.num_clouds))
        dev = lambda t: (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(self.device)
        ops.vote_update_batch(self.votes, self.offsets, outputs, dev(batch.lengths[0]), dev(batch.input_inds),
                              dev(cloud_inds), smooth=self.smooth, is_logits=is_logits, points=points, r2_max=r2_max,
                              labels=None if labels is None else dev(labels),
                              label_values=self.label_values, col_map=self.col_map,
                              confusion=None if labels is None else self._confusion, cloud_inds_host=host)
        return host

    def probs(self, cloud):
        """The [n_cloud_points, C] float64 votes of one cloud (a view of the buffer)."""
        return self.votes[int(self.offsets_host[cloud]):int(self.offsets_host[cloud + 1])]

    def predict(self, cloud, proj=None, targets=None):
        """Raw-label predictions of one cloud, reprojected through proj when given; with targets also its
        [Ctot, Ctot] int64 confusion: (preds, confusion). Device tensors; proj / targets may be arrays."""
        dev = lambda t, dt=None: None if t is None else \
            (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.asarray(t))).to(self.device, dtype=dt)
        return ops.vote_predict(self.probs(cloud), self.label_values, self.col_map, proj=dev(proj),
                                targets=dev(targets, torch.int32))

    def confusion(self, reset=False):
        """The per-batch confusion accumulated by update(labels=...) since the last reset ([Ctot, Ctot] int64)."""
        out = self._confusion.clone()
        if reset:
            self._confusion.zero_()
        return out

    def drop_ignored(self, C):
        """np.delete of the ignored labels' rows and columns (tester.py:242-245)."""
        return np.asarray(C)[self.kept][:, self.kept]


def _val_proportions(dataset, nc_model):
    """Points per kept class over the full validation clouds (tester.py:117-124)."""
    props = np.zeros(nc_model, dtype=np.float32)
    i = 0
    for label_value in dataset.label_values:
        if label_value not in dataset.ignored_labels:
            props[i] = np.sum([np.sum(np.asarray(labels) == label_value) for labels in dataset.validation_labels])
            i += 1
    return props


def _to_device(batch, device):
    if 'cuda' in device.type and hasattr(batch, 'to'):
        batch.to(device)


def cloud_segmentation_validation(net, val_loader, config, accumulator):
    """One validation epoch (trainer.py:338-433): every batch votes into `accumulator` (no radius mask) and its own
    argmax is scored against its labels. Returns the per-class IoUs of the epoch, balanced with the validation
    proportions. The accumulator keeps its votes from one call to the next, as `validation_probs` does."""
    dataset = val_loader.dataset
    was_training = net.training
    net.eval()
    freeze_inference(net)
    accumulator.confusion(reset=True)
    with torch.no_grad():
        for batch in val_loader:
            _to_device(batch, accumulator.device)
            outputs = net(batch, config)
            accumulator.update(batch, outputs, labels=batch.labels)
    C = accumulator.confusion().cpu().numpy().astype(np.int32).astype(np.float32)   # trainer.py:395, :418; kept until the next call
    C = accumulator.drop_ignored(C)
    C *= np.expand_dims(_val_proportions(dataset, accumulator.C) / (np.sum(C, axis=1) + 1e-6), 1)
    IoUs = IoU_from_confusions(C)
    if was_training:
        net.train()             # drops the frozen snapshot
    return IoUs


class ModelTester:

    def __init__(self, net, chkp_path=None, on_gpu=True):
        if on_gpu and torch.cuda.is_available():
            self.device = torch.device("cuda:0")
        else:
            self.device = torch.device("cpu")
        net.to(self.device)
        self.epoch = None
        if chkp_path is not None:
            checkpoint = torch.load(chkp_path, map_location=self.device)
            net.load_state_dict(checkpoint['model_state_dict'])
            self.epoch = checkpoint['epoch']
            print("Model and training state restored.")
        net.eval()
        freeze_inference(net)
        self.accumulator = None
        self.sub_IoUs = self.full_IoUs = None       # the last checkpoint's scores (validation split)
        self.sub_confusion = self.full_confusion = None

    @property
    def test_probs(self):
        """The votes per cloud, device views (the reference's list of host arrays)."""
        return [self.accumulator.probs(i) for i in range(self.accumulator.num_clouds)]

    def cloud_segmentation_test(self, net, test_loader, config, num_votes=30, debug=False):
        """tester.py:79-376: epochs over test_loader until the dataset's minimum potential passes num_votes; sub-cloud
        IoUs whenever it passes the next integer, reprojected full-cloud IoUs (and files, when config.saving) whenever
        its ceiling is a multiple of 10."""
        test_smooth = 0.95
        test_radius_ratio = 0.7
        dataset = test_loader.dataset
        nc_model = config.num_classes
        acc = VoteAccumulator([np.asarray(l).shape[0] for l in dataset.input_labels], nc_model, dataset.label_values,
                              dataset.ignored_labels, self.device, smooth=test_smooth)
        self.accumulator = acc
        label_values = np.asarray(dataset.label_values)

        if config.saving:
            test_path = join('test', config.saving_path.split('/')[-1])
            for sub in ('predictions', 'probs'):
                if not exists(join(test_path, sub)):
                    makedirs(join(test_path, sub))
        else:
            test_path = None

        validation = dataset.set == 'validation'
        val_proportions = _val_proportions(dataset, nc_model) if validation else None
        if validation:          # targets stay in HBM for the whole test
            sub_targets = [torch.as_tensor(np.asarray(l)).to(self.device, dtype=torch.int32) for l in dataset.input_labels]
            full_targets = [torch.as_tensor(np.asarray(l)).to(self.device, dtype=torch.int32)
                            for l in dataset.validation_labels]
        projs = None

        net.eval()
        freeze_inference(net)
        test_epoch = 0
        last_min = -0.5
        t0 = time.time()
        while True:
            with torch.no_grad():
                for i, batch in enumerate(test_loader):
                    _to_device(batch, self.device)
                    outputs = net(batch, config)
                    acc.update(batch, outputs, radius_ratio=test_radius_ratio, in_radius=config.in_radius)

            new_min = float(torch.min(torch.as_tensor(dataset.min_potentials)))
            print('Test epoch {:d}, end. Min potential = {:.1f} ({:.1f}s)'.format(test_epoch, new_min, time.time() - t0))

            if last_min + 1 < new_min:
                last_min += 1

                if validation:
                    print('\nConfusion on sub clouds')
                    conf = torch.zeros((acc.Ctot, acc.Ctot), dtype=torch.int64, device=self.device)
                    for c in range(acc.num_clouds):
                        ops.vote_predict(acc.probs(c), acc.label_values, acc.col_map, targets=sub_targets[c], confusion=conf)
                    self.sub_confusion = conf.cpu().numpy()
                    C = acc.drop_ignored(self.sub_confusion).astype(np.float32)
                    C *= np.expand_dims(val_proportions / (np.sum(C, axis=1) + 1e-6), 1)     # tester.py:248
                    self.sub_IoUs = IoU_from_confusions(C)
                    print(_score_line(self.sub_IoUs) + '\n')

                if int(np.ceil(new_min)) % 10 == 0:
                    print('\nReproject Vote #{:d}'.format(int(np.floor(new_min))))
                    if projs is None:
                        projs = [torch.as_tensor(np.asarray(p)).to(self.device) for p in dataset.test_proj]
                    preds = []
                    conf = torch.zeros((acc.Ctot, acc.Ctot), dtype=torch.int64, device=self.device)
                    for c in range(acc.num_clouds):
                        if validation:
                            p, _ = ops.vote_predict(acc.probs(c), acc.label_values, acc.col_map, proj=projs[c],
                                                    targets=full_targets[c], confusion=conf)
                        else:
                            p = ops.vote_predict(acc.probs(c), acc.label_values, acc.col_map, proj=projs[c])
                        preds.append(p)
                    self.full_preds = preds
                    if validation:
                        print('Confusion on full clouds')
                        self.full_confusion = conf.cpu().numpy()
                        self.full_IoUs = IoU_from_confusions(acc.drop_ignored(self.full_confusion))
                        s = _score_line(self.full_IoUs)
                        print('-' * len(s))
                        print(s)
                        print('-' * len(s) + '\n')

                    if config.saving:
                        print('Saving clouds')
                        for c, file_path in enumerate(dataset.files):
                            points = dataset.load_evaluation_points(file_path)
                            cloud_preds = preds[c].cpu().numpy().astype(np.int32)
                            cloud_name = file_path['scan_id']
                            write_ply(join(test_path, 'predictions', cloud_name), [points, cloud_preds],
                                      ['x', 'y', 'z', 'preds'])
                            # the reprojected votes with a zero column per ignored label (tester.py:273, :287-289, :347-352)
                            proj_probs = acc.probs(c)[projs[c].long()].cpu().numpy()
                            wide = np.zeros((proj_probs.shape[0], acc.Ctot), proj_probs.dtype)
                            wide[:, acc.kept] = proj_probs
                            prob_names = ['_'.join(dataset.label_to_names[label].split()) for label in label_values]
                            write_ply(join(test_path, 'probs', cloud_name), [points, wide], ['x', 'y', 'z'] + prob_names)
                            if dataset.set == 'test':
                                np.savetxt(join(test_path, 'predictions', cloud_name[:-4] + '.txt'), cloud_preds, fmt='%d')

            test_epoch += 1
            if last_min > num_votes:
                break
        return


def _score_line(IoUs):
    s = '{:5.2f} | '.format(100 * np.mean(IoUs))
    for IoU in IoUs:
        s += '{:5.2f} '.format(100 * IoU)
    return s
