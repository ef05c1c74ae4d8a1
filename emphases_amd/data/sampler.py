"""`emphases.data.sampler` (`emphases/data/sampler.py:11-86`): deterministic
variable-size batches of utterances of similar length.  The batches are the
reference's, index for index (tests/golden/loop.npz)."""
import torch

MAX_TRAINING_FRAMES = 75000     # emphases/config/defaults.py:230
RANDOM_SEED = 0                 # defaults.py:116


class Sampler:
    """Batches of indices of `dataset` for one epoch: every bucket of
    `dataset.buckets()` shuffled, cut where one more utterance would take the
    PADDED batch, (items + 1) x the longest, past `max_frames`, the last batch
    of a bucket kept, then all batches shuffled - by a CPU generator seeded
    with `seed + epoch`, which leaves the caller's generator alone.  A
    partition whose name starts with 'test' is walked in order, one utterance
    per batch (`sampler.py:17-22`)."""

    def __init__(self, dataset, max_frames=MAX_TRAINING_FRAMES,
                 seed=RANDOM_SEED):
        partition = getattr(dataset, 'partition', 'train')
        self.sequential = str(partition).startswith('test')
        self.max_frames = max_frames
        self.seed = seed
        self.epoch = 0
        self.length = len(dataset)
        self.buckets = None if self.sequential else dataset.buckets()

    def __iter__(self):
        return iter(self.batch())

    def __len__(self):
        return len(self.batch())

    def set_epoch(self, epoch):
        self.epoch = epoch

    def batch(self):
        """The batches of the current epoch, lists of int."""
        if self.sequential:
            return [[index] for index in range(self.length)]
        generator = torch.Generator()
        generator.manual_seed(self.seed + self.epoch)
        batches = []
        for bucket in self.buckets:
            order = torch.randperm(len(bucket), generator=generator).tolist()
            batch, longest = [], 0
            for index, length in bucket[order].tolist():
                longest = max(longest, length)
                if batch and (len(batch) + 1) * longest > self.max_frames:
                    batches.append(batch)
                    batch, longest = [index], length
                else:
                    batch.append(index)
            if batch:
                batches.append(batch)
        order = torch.randperm(len(batches), generator=generator).tolist()
        return [batches[i] for i in order]
