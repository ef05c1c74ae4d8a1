"""The balanced mel projection of the log-mel front-end (csrc/frontend.hip,
`emph_frontend_mel_plan_fill` / `emph_logmel_planned`): the filterbank's
non-zeros as 16-byte quads dealt evenly over the 64 lanes, every row finished
from at most four partial sums in a fixed order.

Host (no GPU): the plan of the bundled basis, decoded word by word, is the
basis - every non-zero once - within the kernel's bounds.

GPU: the planned kernel against the float64 oracle at the budget of
tests/test_gpu_frontend.py (MARGIN x the float32 floor of
tests/frontend_signals.py, computed on the CPU), on the smallest chunks that
can go wrong: a tile of the kernel is 8 frames, so 7 and 9 frames sit on both
sides of a tile's end, 17 frames leave a tail of one, and 2 frames is the
shortest chunk there is (the reflect pad of 432 needs 433 samples, and 433
samples are 2 frames: a chunk of 1 frame does not exist).  float32 and int16,
mel rows alone (MODE 0) and with the loudness row (MODE 2).  Then what takes no
tolerance: two launches give the same bits, a chunk alone the bits it has
inside a ragged batch, and a basis that has no plan runs one lane per row.
"""
import functools

import numpy as np
import pytest
import torch

import frontend_signals as fs
from emphases_amd import engine as engine_module, melbasis, runtime
from oracle import prominence as oracle

DEVICE = 'cuda:0'
MARGIN = 4.             # tests/test_gpu_frontend.py
SENTINEL = -777.0
QUADS = 5               # csrc/frontend.hip: kQuads
SLOTS = 4               # kPartSlots
MAG_FLOATS = 560        # kMagFloats


###############################################################################
# host: the plan
###############################################################################


def decode(plan):
    """(dense [80, MAG_FLOATS] float64 sum of the plan's weights, hits = how
    many non-zero weights land on each cell, partials per lane [64], lanes per
    row [80]); asserts every index is inside its buffer."""
    assert plan.dtype == np.uint32 and plan.size == (6 * QUADS + 2) * 64
    read = plan[:QUADS * 64].reshape(QUADS, 64).astype(np.int64)
    write = plan[QUADS * 64:2 * QUADS * 64].reshape(QUADS, 64).astype(np.int64)
    weight = plan[2 * QUADS * 64:6 * QUADS * 64].view(np.float32).reshape(
        4 * QUADS, 64)
    restart = plan[6 * QUADS * 64:(6 * QUADS + 1) * 64]
    # the kernel zeroes the magnitudes behind bin 512 only when told to
    assert bool(plan[(6 * QUADS + 1) * 64]) == bool((read + 3 > 512).any())
    assert (read % 4 == 0).all() and (read >= 0).all() and \
        (read + 3 < MAG_FLOATS).all()
    assert (write >= 0).all() and (write < 80 * SLOTS + 64).all()
    dense = np.zeros((80, MAG_FLOATS))
    hits = np.zeros((80, MAG_FLOATS), dtype=np.int64)
    partials = np.zeros(64, dtype=np.int64)
    owners = {}
    for lane in range(64):
        assert not restart[lane] & 1 and restart[lane] < 1 << QUADS
        # a quad's row: the slot its partial is stored to when it closes
        rows, row = [None] * QUADS, None
        for j in reversed(range(QUADS)):
            closes = j == QUADS - 1 or bool(restart[lane] >> (j + 1) & 1)
            if write[j, lane] < 80 * SLOTS:
                assert closes, (lane, j)
                row = int(write[j, lane]) // SLOTS
                owners.setdefault(int(write[j, lane]), []).append(lane)
                partials[lane] += 1
            else:
                # only a quad that closes nothing (or a lane without quads)
                # stores to the lane's spare word
                assert write[j, lane] == 80 * SLOTS + lane
                if closes:
                    row = None
            rows[j] = row
        for j in range(QUADS):
            for i in range(4):
                value = float(weight[4 * j + i, lane])
                if value != 0.:
                    assert rows[j] is not None, (lane, j)
                    dense[rows[j], read[j, lane] + i] += value
                    hits[rows[j], read[j, lane] + i] += 1
    # every slot has one owner, and a row's slots are taken from 0 upwards
    assert all(len(lanes) == 1 for lanes in owners.values())
    lanes = np.zeros(80, dtype=np.int64)
    for slot in owners:
        lanes[slot // SLOTS] += 1
    for row in range(80):
        assert all(SLOTS * row + k in owners for k in range(lanes[row]))
    return dense, hits, partials, lanes


def quads_of(dense):
    """16-byte quads the non-zeros of a dense basis touch, row by row."""
    total = 0
    for row in dense:
        nonzero = np.flatnonzero(row)
        if nonzero.size:
            total += nonzero[-1] // 4 - nonzero[0] // 4 + 1
    return total


def test_plan_of_the_bundled_basis():
    """Every non-zero of the bundled basis exactly once, at most 5 quads and 3
    partial sums per lane, at most 4 lanes per row."""
    basis = melbasis.default()
    plan, counts = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    assert plan is not None
    dense, hits, partials, lanes = decode(plan)
    assert hits.max() == 1 and hits.sum() == basis.nnz == 1001
    assert np.array_equal(dense[:, :513].astype(np.float32), basis.dense)
    assert not dense[:, 513:].any()
    quads, most_quads, most_partials, most_lanes, cycles = (
        int(c) for c in counts)
    print(f'quads {quads}, per lane {most_quads}, partials {most_partials}, '
          f'lanes per row {most_lanes}, read cycles {cycles}')
    assert quads == quads_of(basis.dense) and quads <= 64 * QUADS
    assert most_quads <= QUADS
    assert most_partials == partials.max() <= 3
    assert most_lanes == lanes.max() <= SLOTS
    # the lanes are placed against LDS bank conflicts: no worse than one lane
    # per row, whose nine reads take `read_cycles`
    assert 4 * QUADS <= cycles <= basis.read_cycles
    # the same basis, the same plan
    again, _ = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    assert np.array_equal(plan, again)


def wide_basis():
    """80 rows whose runs are as long as one lane per row takes (20 bins for
    rows 0..63, 40 for rows 64..79): 7 quads a lane."""
    dense = np.zeros((80, 513), dtype=np.float32)
    random = np.random.RandomState(7)
    for row in range(80):
        width = 20 if row < 64 else 40
        low = 1 + 5 * row
        dense[row, low:low + width] = random.uniform(
            0.001, 0.03, width).astype(np.float32)
    return melbasis.SparseBasis(dense, aligned=False)


def nyquist_basis():
    """The bundled basis with a weight on bin 512 (the bundled Nyquist column
    is empty): the one quad that reads behind the magnitudes."""
    dense = melbasis.default().dense.copy()
    assert not dense[:, 512].any() and dense[79, 511] != 0.
    dense[79, 512] = dense[79, 511]
    return melbasis.SparseBasis(dense, aligned=False)


def test_plan_with_a_nyquist_weight():
    bundled_plan, _ = runtime.frontend_mel_plan(*(
        getattr(melbasis.default(), name)
        for name in ('row_start', 'row_count', 'row_offset', 'values')))
    assert not bundled_plan[(6 * QUADS + 1) * 64]
    basis = nyquist_basis()
    plan, _ = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    assert plan[(6 * QUADS + 1) * 64] == 1
    dense, hits, _, _ = decode(plan)
    assert np.array_equal(dense[:, :513].astype(np.float32), basis.dense)
    assert hits.max() == 1 and not dense[:, 513:].any()


def test_basis_without_a_plan():
    """More than 5 quads a lane: no plan (and no error) - the caller runs one
    lane per row."""
    basis = wide_basis()
    assert quads_of(basis.dense) > 64 * QUADS
    plan, counts = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    assert plan is None and counts is None


def test_plan_of_a_sparse_basis():
    """Empty rows, one-bin rows and a lane without quads: still the basis."""
    dense = np.zeros((80, 513), dtype=np.float32)
    dense[3, 7] = 0.5
    dense[4, 8:13] = 0.25
    dense[79, 500:513] = 0.125
    basis = melbasis.SparseBasis(dense, aligned=False)
    plan, counts = runtime.frontend_mel_plan(
        basis.row_start, basis.row_count, basis.row_offset, basis.values)
    got, hits, _, lanes = decode(plan)
    assert np.array_equal(got[:, :513].astype(np.float32), dense)
    assert hits.max() == 1 and hits.sum() == 19 and int(counts[0]) == 7
    assert lanes.sum() == lanes[[3, 4, 79]].sum()


###############################################################################
# GPU
###############################################################################


@pytest.fixture(scope='module')
def engine():
    return engine_module.Engine(device=0)


def budget():
    """(mel, dB) budgets, raw: MARGIN x the floors tests/test_gpu_frontend.py
    computes (once per session, shared with it)."""
    from test_gpu_frontend import floors
    table = floors()
    return MARGIN * table['mel', False], MARGIN * table['db', False]


class Basis:
    """A filterbank on the device with its plan (None: it has none)."""

    def __init__(self, basis):
        to = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEVICE)  # noqa: E731
        self.dense = torch.from_numpy(basis.dense)
        self.start, self.count, self.offset, self.values = (
            to(a) for a in (basis.row_start, basis.row_count,
                            basis.row_offset, basis.values))
        self.nnz = int(basis.values.size)
        plan, _ = runtime.frontend_mel_plan(
            basis.row_start, basis.row_count, basis.row_offset, basis.values)
        self.plan = None if plan is None else to(plan.view(np.int32))


@functools.lru_cache(maxsize=None)
def bundled():
    return Basis(melbasis.default())


def device_audio(pcm, fmt):
    host = pcm if fmt == 'int16' else fs.as_float(pcm)
    return torch.from_numpy(host).to(DEVICE)


def launch(engine, basis, audio, lengths, mode, planned=True, lead=5, gap=3):
    """`emph_logmel_planned` (MODE 2: `emph_frontend_peak` first) over whole
    utterances of `lengths` samples packed back to back in `audio`, `gap`
    sentinel columns apart from column `lead`.  Returns (out [rows, ld] on the
    host, frame_off, frames)."""
    lib = runtime.library()
    table = np.zeros((len(lengths), runtime.SEG_FIELDS), dtype=np.int64)
    tiles, cursor, offset = [], lead, 0
    for index, length in enumerate(lengths):
        frames = fs.frames_of(length)
        table[index, runtime.SEG_AUDIO_OFF] = offset
        table[index, runtime.SEG_AUDIO_LEN] = length
        table[index, runtime.SEG_START] = 432
        table[index, runtime.SEG_LENGTH] = length
        table[index, runtime.SEG_FRAME_OFF] = cursor
        table[index, runtime.SEG_FRAMES] = frames
        tiles += [(index, first, cursor, frames) for first in range(0, frames, 8)]
        cursor += frames + gap
        offset += length
    ld = cursor + 8
    tiles = np.array(tiles, dtype=np.int32)
    seg_dev = torch.from_numpy(table).to(DEVICE)
    tiles_dev = torch.from_numpy(tiles).to(DEVICE)
    peak = torch.zeros(len(lengths), dtype=torch.float32, device=DEVICE)
    form = engine_module.audio_format(audio)
    if mode == 2:
        runtime.check(lib.emph_frontend_peak(
            audio.data_ptr(), form, seg_dev.data_ptr(), tiles_dev.data_ptr(),
            len(tiles), engine.table.data_ptr(), peak.data_ptr(), None),
            'emph_frontend_peak')
    rows = {0: 80, 2: 81}[mode]
    out = torch.full((rows, ld), SENTINEL, device=DEVICE)
    plan = basis.plan if planned else None
    runtime.check(lib.emph_logmel_planned(
        audio.data_ptr(), form, seg_dev.data_ptr(), tiles_dev.data_ptr(),
        len(tiles), engine.table.data_ptr(), basis.start.data_ptr(),
        basis.count.data_ptr(), basis.offset.data_ptr(),
        basis.values.data_ptr(), basis.nnz,
        None if plan is None else plan.data_ptr(), out.data_ptr(), ld, 0,
        80 if mode == 2 else -1, peak.data_ptr() if mode == 2 else None,
        engine.a_weights.data_ptr(), 0, None), 'emph_logmel_planned')
    out = out.cpu()
    frame_off = table[:, runtime.SEG_FRAME_OFF]
    frames = table[:, runtime.SEG_FRAMES]
    inside = np.zeros(ld, dtype=bool)
    for off, count in zip(frame_off, frames):
        inside[off:off + count] = True
    inside = torch.from_numpy(inside)
    assert bool((out[:, ~inside] == SENTINEL).all())
    assert bool(torch.isfinite(out[:, inside]).all())
    return out, frame_off, frames


# samples of the chunks: 2, 7, 9 frames; 2, 8 and 17 frames side by side (odd
# lengths: the chunks behind the first start on odd samples)
SHAPES = {'frames2': (433,), 'frames7': (160 * 7 + 3,), 'frames9': (160 * 9 + 5,),
          'ragged': (433, 160 * 8 + 1, 160 * 17 + 7)}
assert [[fs.frames_of(n) for n in shape] for shape in SHAPES.values()] == \
    [[2], [7], [9], [2, 8, 17]]


@functools.lru_cache(maxsize=None)
def chunks_of(shape):
    """[(int16 [S], its float64 oracle: mel [80, F], loudness [F])]: the chirp
    where it sweeps through the middle rows, the full-scale noise, a speech-like
    signal."""
    signals = fs.signals()
    sources = [signals['chirp'][160 * 600:], signals['noise_full'],
               signals['synth61'][160 * 90:]]
    out = []
    for index, length in enumerate(SHAPES[shape]):
        pcm = np.ascontiguousarray(sources[index % 3][:length])
        audio = fs.as_double(pcm)
        out.append((pcm, audio, oracle.mel(audio),
                    oracle.loudness_of_power(oracle.power(audio))[0]))
    return out


def mel_gap(rows, audio, want, dense=None):
    """The metric of tests/frontend_signals.py (`mel_error`); `dense`: of a
    basis other than the bundled one."""
    if dense is None:
        return float(fs.mel_error(rows, audio, False, want).max())
    scale = dense.double().sum(dim=1)[:, None] * \
        (fs.frame_norms(audio)[None] + 1e-3)
    return float(((fs.mel_of_log(rows, False) - want).abs() / scale).max())


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [0, 2])
@pytest.mark.parametrize('fmt', ['float32', 'int16'])
@pytest.mark.parametrize('shape', list(SHAPES))
def test_planned_against_oracle(engine, shape, fmt, mode):
    """The planned kernel on the smallest chunks against the float64 oracle;
    twice: the same bits."""
    basis = bundled()
    assert basis.plan is not None and engine.mel_plan is not None
    chunks = chunks_of(shape)
    audio = device_audio(np.concatenate([c[0] for c in chunks]), fmt)
    out, frame_off, frames = launch(
        engine, basis, audio, SHAPES[shape], mode)
    mel_budget, db_budget = budget()
    for index, (_, double, want, loudness) in enumerate(chunks):
        piece = out[:, frame_off[index]:frame_off[index] + frames[index]]
        gap = mel_gap(piece[:80], double, want)
        print(f'{shape}[{index}] {fmt} mode {mode}: mel {gap:.2e} / floor = '
              f'{gap / (mel_budget / MARGIN):.2f}')
        assert gap < mel_budget
        if mode == 2:
            gap = float((piece[80].double() - loudness).abs().max())
            print(f'{shape}[{index}] {fmt} mode {mode}: db {gap:.2e} / floor '
                  f'= {gap / (db_budget / MARGIN):.2f}')
            assert gap < db_budget
    again, _, _ = launch(engine, basis, audio, SHAPES[shape], mode)
    assert torch.equal(out, again)


@pytest.mark.gpu
@pytest.mark.parametrize('fmt', ['float32', 'int16'])
def test_alone_equals_in_batch(engine, fmt):
    """Each chunk of the ragged batch launched alone (at another frame offset)
    has the bits it has inside the batch; int16 and float32 give the same
    bits; the loudness row does not depend on the mel rows' mapping."""
    basis = bundled()
    chunks = chunks_of('ragged')
    lengths = SHAPES['ragged']
    audio = device_audio(np.concatenate([c[0] for c in chunks]), fmt)
    both, frame_off, frames = launch(engine, basis, audio, lengths, 2)
    for index, (pcm, _, _, _) in enumerate(chunks):
        alone, off, count = launch(
            engine, basis, device_audio(pcm, fmt), lengths[index:index + 1], 2,
            lead=16)
        assert torch.equal(
            alone[:, off[0]:off[0] + count[0]],
            both[:, frame_off[index]:frame_off[index] + frames[index]])
    if fmt == 'int16':
        other, _, _ = launch(
            engine, basis,
            device_audio(np.concatenate([c[0] for c in chunks]), 'float32'),
            lengths, 2)
        assert torch.equal(both, other)
    rows, _, _ = launch(engine, basis, audio, lengths, 2, planned=False)
    assert torch.equal(rows[80], both[80])
    # the two mappings add the same products in another order
    assert not torch.equal(rows[:80], both[:80])
    assert float((rows[:80] - both[:80]).abs().max()) < 1e-4


@pytest.mark.gpu
def test_planned_nyquist_weight(engine):
    """A weight on bin 512: its quad reads three floats behind the magnitudes,
    which the kernel then zeroes (0 x the spectrum's bits could be NaN).  The
    full-scale noise has energy there; against the float64 oracle of that
    basis, and the other rows the bits of the bundled basis."""
    basis = Basis(nyquist_basis())
    assert basis.plan is not None
    chunks = chunks_of('ragged')
    lengths = SHAPES['ragged']
    audio = device_audio(np.concatenate([c[0] for c in chunks]), 'float32')
    out, frame_off, frames = launch(engine, basis, audio, lengths, 0)
    mel_budget, _ = budget()
    for index, (_, double, _, _) in enumerate(chunks):
        piece = out[:, frame_off[index]:frame_off[index] + frames[index]]
        want = oracle.mel(double, basis.dense)
        gap = mel_gap(piece, double, want, basis.dense)
        print(f'nyquist[{index}]: mel {gap:.2e} / floor = '
              f'{gap / (mel_budget / MARGIN):.2f}')
        assert gap < mel_budget
    plain, _, _ = launch(engine, bundled(), audio, lengths, 0)
    assert torch.equal(out[:79], plain[:79])
    assert not torch.equal(out[79], plain[79])


@pytest.mark.gpu
@pytest.mark.parametrize('mode', [0, 2])
def test_basis_without_a_plan_runs_one_lane_per_row(engine, mode):
    """A basis of 7 quads a lane has no plan: `emph_logmel_planned` runs it
    one lane per row, `emph_logmel`'s bits, within the budget of its own
    float64 oracle."""
    basis = Basis(wide_basis())
    assert basis.plan is None
    chunks = chunks_of('ragged')
    lengths = SHAPES['ragged']
    audio = device_audio(np.concatenate([c[0] for c in chunks]), 'float32')
    out, frame_off, frames = launch(engine, basis, audio, lengths, mode)
    mel_budget, _ = budget()
    for index, (_, double, _, _) in enumerate(chunks):
        piece = out[:80, frame_off[index]:frame_off[index] + frames[index]]
        want = oracle.mel(double, basis.dense)
        gap = mel_gap(piece, double, want, basis.dense)
        print(f'wide[{index}] mode {mode}: mel {gap:.2e} / floor = '
              f'{gap / (mel_budget / MARGIN):.2f}')
        assert gap < mel_budget
    if mode == 2:
        # the loudness row does not know the basis
        same, _, _ = launch(engine, bundled(), audio, lengths, 2)
        assert torch.equal(out[80], same[80])
