"""The variance baselines on the MI355X: `emph_quantile_spreads` bitwise against
torch.quantile on the CPU, pitch- and duration-variance against the
reference's goldens (tests/golden/baselines.npz), and the METHOD switch
through every entry point."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import emphases_amd
from emphases_amd import Config, alignment as alignment_module, load, runtime
from emphases_amd.baselines import pitch_variance

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_baselines import duration_alignments, split  # noqa: E402


@pytest.fixture(scope='module')
def golden():
    with np.load(os.path.join(HERE, 'golden', 'baselines.npz')) as data:
        return {key: data[key] for key in data.files}


def quantiles(x):
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    q05, q95 = torch.quantile(x, .05), torch.quantile(x, .95)
    return np.array([q05, q95, q95 - q05], dtype=np.float32)


def same_bits(got, want):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.int32), want[~nan].view(np.int32))


def test_spread_kernel_bitwise_against_torch_quantile():
    rng = np.random.default_rng(7)
    lengths = list(rng.integers(1, 5001, 500)) + [
        1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096,
        4097, 30000, (1 << 20) + 3]
    rows = []
    for index, n in enumerate(lengths):
        x = rng.normal(0., 2., int(n)).astype(np.float32)
        kind = index % 6
        if kind == 1:
            x = np.round(x * 64.) / 64.         # ties
        elif kind == 2:
            x[rng.choice(n, max(1, n // 50))] = np.inf
            x[rng.choice(n, max(1, n // 50))] = -np.inf
        elif kind == 3:
            x[rng.choice(n, max(1, n // 4))] = -np.inf
        elif kind == 4 and index % 12 == 4:
            x[rng.integers(0, n)] = np.nan
        elif kind == 5:
            x = np.round(x).astype(np.float32)  # heavy ties
        x[x == 0] = 0.                          # (no -0: torch keeps either zero)
        rows.append(x)
    sizes = np.array([len(x) for x in rows], dtype=np.int64)
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    count = len(rows)
    # every segment is a "word" of one of the last three, which are "utterances"
    table = np.stack([offsets[:-1], sizes, count - 3 + np.arange(count) % 3],
                     axis=1)
    table[-3:, 2] = -1
    values = torch.from_numpy(np.concatenate(rows)).cuda()
    stats, scores, _ = pitch_variance.quantile_spreads(values, table, count - 3)
    stats, scores = stats.cpu().numpy(), scores.cpu().numpy()
    want = np.stack([quantiles(x) for x in rows])
    same_bits(stats, want)
    expect = (torch.from_numpy(want[:-3, 2]) -
              torch.from_numpy(want[count - 3 + np.arange(count - 3) % 3, 2]))
    same_bits(scores, expect.numpy())
    # deterministic
    again, _, _ = pitch_variance.quantile_spreads(values, table, count - 3)
    same_bits(again.cpu().numpy(), stats)


def golden_tracker(golden):
    rows = dict(zip(golden['pv_frames'].tolist(),
                    split(golden['pv_pitch'], golden['pv_frames'])))

    def track(audio):
        pitch = torch.from_numpy(rows[audio.shape[-1] // 160].copy())[None]
        return pitch, torch.ones_like(pitch)
    return track


def pitch_alignments(golden):
    return [alignment_module.Alignment(
        [alignment_module.Word(f'w{i}', a, b) for i, (a, b) in enumerate(t)])
        for t in split(golden['pv_times'], golden['pv_words'])]


def test_pitch_variance_against_reference(golden):
    tracker = golden_tracker(golden)
    alignments = pitch_alignments(golden)
    audios = [torch.zeros(1, 160 * int(n)) for n in golden['pv_frames']]
    got = emphases_amd.from_alignments_and_audios(
        alignments, audios, gpu=0, config=Config(method='pitch-variance'),
        pitch_tracker=tracker)
    want = split(golden['pv_scores'], golden['pv_words'])
    for a, b in zip(got, want):
        assert a.is_cuda and a.dtype == torch.float32 and a.shape == (1, len(b))
        a = a[0].cpu().numpy()
        nan = np.isnan(b)
        assert np.array_equal(np.isnan(a), nan)
        assert np.abs(a[~nan] - b[~nan]).max(initial=0.) <= 4e-6
    # the values the kernel selected over (log2 on the device): bitwise
    rows = [torch.from_numpy(p) for p in
            split(golden['pv_pitch'], golden['pv_frames'])]
    frames = [int(n) for n in golden['pv_frames']]
    times = split(golden['pv_times'], golden['pv_words'])
    table = pitch_variance.segment_table(times, frames)
    stats, scores, chosen = pitch_variance.quantile_spreads(
        torch.cat(rows).cuda(), table, len(golden['pv_times']),
        runtime.SPREAD_LOG2, selected=True)
    chosen, stats = chosen.cpu().numpy(), stats.cpu().numpy()
    want = np.stack([quantiles(chosen[a:a + n]) for a, n, _ in table])
    same_bits(stats, want)
    same_bits(scores.cpu().numpy(),
              (torch.from_numpy(want[:-len(frames), 2]) -
               torch.from_numpy(want[table[:-len(frames), 2], 2])).numpy())
    # an empty word raises torch's error before anything is launched
    with runtime.LaunchTimer() as timer:
        with pytest.raises(RuntimeError, match='must be non-empty'):
            pitch_variance.infer(
                emphases_amd.Alignment.from_frames(np.array([[400], [500]])),
                torch.zeros(1, 160 * 300), 16000, gpu=0,
                pitch_tracker=tracker)
        assert timer.count() == 0


def test_duration_variance_on_device(golden):
    alignments = duration_alignments(golden)
    got = emphases_amd.from_alignments_and_audios(
        alignments, [None] * len(alignments), gpu=0,
        config=Config(method='duration-variance'))
    for a, b in zip(got, split(golden['dv_scores'], golden['dv_words'])):
        assert a.is_cuda
        same_bits(a[0].cpu().numpy(), b)


def synthetic_tracker(audio):
    """Deterministic stand-in for penn: one frame per 160 samples, 0 Hz where
    the signal is silent (-inf after log2)."""
    pitch = (60. + 400. * audio.reshape(-1)[::160].abs()).to(torch.float32)
    pitch[audio.reshape(-1)[::160] == 0] = 0.
    return pitch[None], torch.ones_like(pitch)[None]


def write_corpus(directory, count):
    """<directory>/u<i>.wav (16-bit PCM; every 7th at 8 kHz, every 11th at
    22.05 kHz) + u<i>.TextGrid with a phones tier."""
    from emphases_amd import synth
    frames = synth.corpus_frames(count, 200, 3000)
    texts, waves = [], []
    for index, n in enumerate(frames):
        rate = 8000 if index % 7 == 3 else 22050 if index % 11 == 5 else 16000
        audio = synth.weights(700 + index, (1, int(n) * rate // 100), 0.3)
        bounds = synth.word_frames(500 + index, int(n))
        words = []
        for k, (a, b) in enumerate(bounds.T):
            a, b = int(a) / 100., int(b) / 100.
            parts = 1 + (k % 5)
            step = (b - a) / parts
            words.append(alignment_module.Word(f'w{k}', a, b, [
                alignment_module.Phoneme(f'p{j}', a + j * step,
                                         b if j == parts - 1 else
                                         a + (j + 1) * step)
                for j in range(parts)]))
        texts.append(os.path.join(directory, f'u{index}.TextGrid'))
        waves.append(os.path.join(directory, f'u{index}.wav'))
        alignment_module.Alignment(words).save(texts[-1])
        load.save_wav(waves[-1], audio, rate)
    return texts, waves


def _free_port():
    with socket.socket() as sock:
        sock.bind(('127.0.0.1', 0))
        return sock.getsockname()[1]


@pytest.mark.timeout(900)
def test_method_reaches_every_entry_point(tmp_path):
    sys.path.insert(0, HERE)
    import dist_worker
    count = 60
    aligns, audios = dist_worker.corpus(count, 200, 3000)
    pitch = Config(method='pitch-variance')
    batch = emphases_amd.from_alignments_and_audios(
        aligns, audios, gpu=0, config=pitch, pitch_tracker=synthetic_tracker)
    alone = emphases_amd.from_alignments_and_audios(
        aligns[7:8], audios[7:8], gpu=0, config=pitch,
        pitch_tracker=synthetic_tracker)[0]
    assert torch.equal(alone, batch[7])
    assert torch.isfinite(torch.cat([b[0] for b in batch])).float().mean() > .5
    previous = emphases_amd.active_config()
    try:
        emphases_amd.configure(method='pitch-variance')
        one = emphases_amd.from_alignment_and_audio(
            aligns[7], audios[7], 16000, gpu=0,
            pitch_tracker=synthetic_tracker)
        assert torch.equal(one, batch[7])
        # files at 16 / 8 / 22.05 kHz
        directory = tmp_path / 'corpus'
        directory.mkdir()
        texts, waves = write_corpus(str(directory), count)
        prefixes = [str(directory / f'pv_{i}') for i in range(count)]
        emphases_amd.from_files_to_files(
            texts, waves, prefixes, gpu=0, utterances_per_batch=16,
            pitch_tracker=synthetic_tracker)
        saved = [torch.load(f'{p}.pt') for p in prefixes]
        for index in (0, 3, 5, 16, count - 1):
            got = emphases_amd.from_file(texts[index], waves[index], gpu=0,
                                         pitch_tracker=synthetic_tracker)
            assert torch.equal(got.cpu(), saved[index])
        emphases_amd.from_file_to_file(
            texts[5], waves[5], str(directory / 'one'), gpu=0,
            pitch_tracker=synthetic_tracker)
        assert torch.equal(torch.load(directory / 'one.pt'), saved[5])
        # duration-variance through the files API
        emphases_amd.configure(method='duration-variance')
        durations = [str(directory / f'dv_{i}') for i in range(count)]
        emphases_amd.from_files_to_files(texts, waves, durations, gpu=0)
        expect = emphases_amd.from_alignments_and_audios(
            [emphases_amd.Alignment(t) for t in texts], [None] * count)
        for prefix, want in zip(durations, expect):
            assert torch.equal(torch.load(f'{prefix}.pt'), want)
    finally:
        emphases_amd.configure(previous)
    assert emphases_amd.active_config().method == 'neural'
    # the command line
    few = 12
    child = subprocess.run(
        [sys.executable, '-m', 'emphases_amd', '--text_files', *texts[:few],
         '--audio_files', *waves[:few], '--output_prefixes',
         *[str(directory / f'cli_{i}') for i in range(few)], '--gpu', '0',
         '--method', 'duration-variance'], cwd=ROOT, timeout=600)
    assert child.returncode == 0
    for index in range(few):
        assert torch.equal(torch.load(directory / f'cli_{index}.pt'),
                           expect[index])
    # two gloo ranks
    port = _free_port()
    children = []
    for rank in range(2):
        env = dict(os.environ, RANK=str(rank), LOCAL_RANK=str(rank),
                   WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port))
        out = tmp_path / f'rank{rank}.pt'
        ranked = [str(directory / f'r2_{i}') for i in range(count)]
        children.append((out, subprocess.Popen(
            [sys.executable, os.path.join(HERE, 'baselines_worker.py'),
             'duration-variance', str(out), *texts, '--', *waves, '--',
             *ranked], env=env, cwd=ROOT)))
    for out, child in children:
        assert child.wait(timeout=600) == 0
        for got, want in zip(torch.load(out), expect):
            assert torch.equal(got, want)
    for index in range(count):
        assert torch.equal(torch.load(directory / f'r2_{index}.pt'),
                           expect[index])
