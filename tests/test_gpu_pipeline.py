"""The two users of `emphases_amd.pipeline` at the same time in one process:
the shared file pool is placed once and both calls write what they write
alone."""
import threading

import pytest

import emphases_amd as emphases
from emphases_amd import load, synth
from emphases_amd.data.preprocess import core as preprocess

pytestmark = pytest.mark.gpu


def test_preprocessing_beside_inference_writes_the_same_bytes(tmp_path):
    """`data.preprocess.from_files_to_files` and `from_files_to_files` over the
    same 48 ragged 16-bit PCM files, each alone and then both at once on two
    threads: every output file of the overlapping runs (`.pt` of mels,
    loudness and scores, `.TextGrid`) is byte for byte the solo run's."""
    count, per_batch = 48, 8
    frames = synth.integers(5201, count, 60, 900)
    texts, waves = [], []
    for index, length in enumerate(frames):
        waves.append(tmp_path / f'u{index}.wav')
        audio = synth.audio(index, int(length))
        load.save_wav(waves[-1], audio[:, :audio.shape[1] - index % 7])
        texts.append(tmp_path / f'u{index}.TextGrid')
        emphases.Alignment.from_frames(
            synth.word_frames(index, int(length) - 1)).save(texts[-1])

    def features(out):
        preprocess.from_files_to_files(
            waves, [out / f'm{i}.pt' for i in range(count)],
            [out / f'l{i}.pt' for i in range(count)], gpu=0,
            files_per_batch=per_batch)

    def scores(out):
        out.mkdir()
        emphases.from_files_to_files(
            texts, waves, [out / f's{i}' for i in range(count)], gpu=0,
            utterances_per_batch=per_batch)

    def snapshot(out):
        return {path.name: path.read_bytes() for path in sorted(out.iterdir())}

    features(tmp_path / 'features_alone')
    scores(tmp_path / 'scores_alone')
    alone = (snapshot(tmp_path / 'features_alone'),
             snapshot(tmp_path / 'scores_alone'))
    assert len(alone[0]) == 2 * count and len(alone[1]) == 2 * count

    for lap in range(3):
        outs = tmp_path / f'features_{lap}', tmp_path / f'scores_{lap}'
        barrier, errors = threading.Barrier(2), []

        def work(call, out):
            try:
                barrier.wait(30)
                call(out)
            except BaseException as error:      # noqa: BLE001
                errors.append(error)

        threads = [threading.Thread(target=work, args=pair)
                   for pair in zip((features, scores), outs)]
        for thread in threads:
            thread.start()
        for thread in threads:
            thread.join()
        assert errors == []
        assert (snapshot(outs[0]), snapshot(outs[1])) == alone, lap
    assert not [thread.name for thread in threading.enumerate()
                if thread.name.startswith('emphases-')]
