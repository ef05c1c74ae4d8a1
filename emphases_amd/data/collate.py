"""`emphases.data.collate` (`emphases/data/collate.py:11-78`) on the device:
where the reference pads the items of a batch into host tensors, one
`emph_collate` launch copies them out of the resident dataset straight into
the packed ragged layout of the batch's plan."""
import numpy as np
import torch

from .. import runtime


def item_table(dataset, indices, plan):
    """int64 [items, 6] of `emph_collate`: where every item lies in the
    resident arrays and where the plan puts it."""
    indices = np.asarray(indices, dtype=np.int64)
    # (the kernel finds a column's item by bisection over the packed columns)
    assert np.all(np.diff(plan.frame_off) >= 0) and \
        np.all(np.diff(plan.word_off) >= 0)
    return np.ascontiguousarray(np.stack([
        dataset.frame_first[indices], dataset.lengths[indices],
        plan.frame_off, dataset.word_first[indices], dataset.words[indices],
        plan.word_off], axis=1), dtype=np.int64)


def collate(dataset, indices, plan, features, targets):
    """Fill `features` [C, plan.ld_frames] and `targets` [plan.ld_words]
    (float32 device tensors that may hold anything) with the batch `indices`
    of `dataset`: every column is written, zero where the plan has no data."""
    channels = dataset.features.shape[0]
    assert features.shape == (channels, plan.ld_frames) and \
        targets.shape == (plan.ld_words,)
    assert features.is_contiguous() and features.dtype == torch.float32
    assert targets.is_contiguous() and targets.dtype == torch.float32
    with torch.cuda.device(dataset.device):
        table = torch.from_numpy(
            item_table(dataset, indices, plan)).to(dataset.device)
        runtime.check(runtime.library().emph_collate(
            dataset.features.data_ptr(), dataset.features.shape[1],
            dataset.targets.data_ptr(), dataset.targets.numel(),
            table.data_ptr(), table.shape[0], channels, plan.ld_frames,
            plan.ld_words, features.data_ptr(), targets.data_ptr(),
            runtime.stream()), 'emph_collate')
    return features, targets
