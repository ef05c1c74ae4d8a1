"""Between what callers hold - columns back to back, or a padded `[B, C, T]`
batch - and the library's packed axes (`batch.Plan`: every segment starts on
a multiple of 16 columns, zeros between).  One indexed copy each way, not one
slice per segment: 64 segments cost 0.5 ms of launches (tools/ops_cost.py).
What `core`'s step functions and `ops` share."""
import numpy as np
import torch


def column_index(offsets, counts):
    """int64 [sum(counts)]: the packed columns of segments of `counts[i]`
    positions that start at column `offsets[i]`, in segment order."""
    offsets = np.asarray(offsets, dtype=np.int64)
    counts = np.asarray(counts, dtype=np.int64)
    first = np.cumsum(counts) - counts
    return np.repeat(offsets - first, counts) + \
        np.arange(int(counts.sum()), dtype=np.int64)


def columns(offsets, counts, device):
    """`column_index` on `device`."""
    return torch.from_numpy(column_index(offsets, counts)).to(device)


def scatter(x, columns, ld):
    """Back-to-back columns -> the library's packed axis, zeros between.  The
    way back is `packed.index_select(1, columns)`."""
    packed = torch.zeros((x.shape[0], ld), dtype=torch.float32,
                         device=x.device)
    packed.index_copy_(1, columns, x[:, :columns.numel()].to(torch.float32))
    return packed


class Padded:
    """A padded batch `[B, C, T]` (item i valid up to its own length) against
    the packed axes of its `plan`: the plan's integer metadata on the device
    with named views, `pack` onto an axis and `unpack` from one.  The columns
    behind an item's length are never read and come back as zeros."""

    def __init__(self, plan, device, tile_requests=()):
        self.plan, self.device = plan, device
        self._requests = list(tile_requests)
        self._meta = None
        self._index = None

    def view(self, name):
        """Piece `name` of `Plan.pack_metadata` (with the tile tables asked
        for) on the device; uploaded when first asked for."""
        if self._meta is None:
            host, self._offsets = self.plan.pack_metadata(self._requests)
            self._meta = torch.from_numpy(host).to(self.device)
        start, size = self._offsets[name]
        return self._meta[start:start + size]

    def _axis(self, axis):
        """((item, position in the item, packed column) of every valid
        position of `axis` - 'frames' or 'words' - on the device, the leading
        dimension of the axis); both axes travel in one upload."""
        plan = self.plan
        if self._index is None:
            host = []
            for offsets, counts in ((plan.frame_off, plan.frames),
                                    (plan.word_off, plan.words)):
                first = np.cumsum(counts) - counts
                item = np.repeat(np.arange(len(counts), dtype=np.int64), counts)
                host.append(np.stack([
                    item, np.arange(len(item), dtype=np.int64) - first[item],
                    column_index(offsets, counts)]))
            both = torch.from_numpy(np.concatenate(host, axis=1)).to(
                self.device)
            cut = host[0].shape[1]
            self._index = {'frames': (both[:, :cut], plan.ld_frames),
                           'words': (both[:, cut:], plan.ld_words)}
        return self._index[axis]

    def pack(self, xs, axis):
        """float32 `[C, ld]` on the device: item i's valid columns of `xs`
        `[B, C, T]` at its place on the packed `axis`."""
        (item, position, column), ld = self._axis(axis)
        xs = xs.to(self.device, torch.float32)
        return scatter(xs[item, :, position].t(), column, ld)

    def unpack(self, packed, axis, width):
        """float32 `[B, C, width]`: the way back from `packed` `[C, ld]`."""
        (item, position, column), _ = self._axis(axis)
        result = torch.zeros(
            (len(self.plan), packed.shape[0], width), dtype=torch.float32,
            device=self.device)
        result[item, :, position] = packed.index_select(1, column).t()
        return result
