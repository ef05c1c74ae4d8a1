"""`emphases.data.loader` (`emphases/data/loader.py:11-25`): batches of a
resident `Dataset` in the order of a `Sampler`, as the prepared
`train.Batch` objects `Trainer.step` takes."""
import torch

from .. import core as api
from .collate import collate as device_collate


class Loader:
    """Iterating yields one `train.Batch` per batch of `sampler`.  The plan
    and its metadata are made on the host from the dataset's arrays, the way
    `Trainer.prepare` makes them from a collated batch; the data comes from
    one `emph_collate` launch into buffers the loader owns.  Two sets of
    buffers alternate: a batch stays valid until the one after the next is
    built."""

    def __init__(self, dataset, sampler, trainer):
        if dataset.features is None:
            raise ValueError('the dataset is not on the device (upload())')
        if dataset.device != trainer.device:
            raise ValueError(
                f'the dataset is on {dataset.device}, the trainer on '
                f'{trainer.device}')
        if dataset.features.shape[0] != trainer.config.num_features:
            raise ValueError(
                f'the dataset holds {dataset.features.shape[0]} features, '
                f'the model takes {trainer.config.num_features}')
        self.dataset, self.sampler, self.trainer = dataset, sampler, trainer
        self.batch_sampler = sampler        # (the reference's DataLoader name)
        self._slots = [[None, None], [None, None]]
        self._next = 0

    def __len__(self):
        return len(self.sampler)

    def __iter__(self):
        for indices in self.sampler:
            yield self.batch(indices)

    def _buffer(self, slot, which, size):
        found = self._slots[slot][which]
        if found is None or found.numel() < size:
            found = torch.empty(
                size, dtype=torch.float32, device=self.dataset.device)
            self._slots[slot][which] = found
        return found[:size]

    def batch(self, indices):
        """The prepared batch of the utterances `indices`."""
        from .. import train
        dataset = self.dataset
        indices = [int(index) for index in indices]
        plan = api._packed_plan(
            dataset.lengths[indices],
            [torch.from_numpy(dataset.word_bounds(i)) for i in indices],
            dataset.words[indices])
        meta = self.trainer.metadata(plan)
        slot, self._next = self._next, 1 - self._next
        channels = dataset.features.shape[0]
        with torch.cuda.device(dataset.device):
            features = self._buffer(
                slot, 0, channels * plan.ld_frames).view(
                    channels, plan.ld_frames)
            targets = self._buffer(slot, 1, plan.ld_words)
        device_collate(dataset, indices, plan, features, targets)
        return train.Batch(plan, meta, features, targets)
