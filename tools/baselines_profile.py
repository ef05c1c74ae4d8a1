"""Device time of the pitch-variance kernels and files/s of the duration-variance
file API (measurement only).

    python tools/baselines_profile.py [--files N] [--out DIR]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/baselines_profile.py

pitch-variance on BASELINE configs[1] shapes (64 x 10 s: 64 000 frames) and
configs[4] shapes (64 x 5 min: 1.92 M frames) with a seeded pitch stand-in,
timed per launch by the library's kernel-exact timer (`runtime.LaunchTimer`);
then `from_files_to_files` on N (default 4 096) 10 s files with a phones tier,
method 'duration-variance' beside 'neural', on the same files.  One JSON line.
"""
import argparse
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import emphases_amd  # noqa: E402
from emphases_amd import Config, alignment as alignment_module  # noqa: E402
from emphases_amd import load, runtime, synth  # noqa: E402


def tracker(audio):
    frames = -(-audio.shape[-1] // 160)
    rng = np.random.default_rng(frames)
    pitch = 150. * np.exp2(rng.normal(0., .3, frames))
    return (torch.from_numpy(pitch.astype(np.float32))[None],
            torch.ones(1, frames))


def pitch_variance(utterances, frames, repeats=5):
    audios = [torch.zeros(1, frames * 160) for _ in range(utterances)]
    aligns = [emphases_amd.Alignment.from_frames(
        synth.word_frames(100 + i, frames)) for i in range(utterances)]
    config = Config(method='pitch-variance')
    emphases_amd.from_alignments_and_audios(
        aligns, audios, gpu=0, config=config, pitch_tracker=tracker)
    launches = []
    for _ in range(repeats):
        with runtime.LaunchTimer() as timer:
            emphases_amd.from_alignments_and_audios(
                aligns, audios, gpu=0, config=config, pitch_tracker=tracker)
        launches.append(timer.microseconds.tolist())
    spreads = [run[0] for run in launches]
    differences = [run[1] for run in launches]
    return {'utterances': utterances, 'frames': utterances * frames,
            'words': int(sum(len(a) for a in aligns)),
            'spread_us_median': float(np.median(spreads)),
            'difference_us_median': float(np.median(differences)),
            'launches_per_call': len(launches[0])}


def corpus(directory, count):
    texts, waves = [], []
    audio = synth.audio(1, 1000)
    for index in range(count):
        bounds = synth.word_frames(500 + index, 1000)
        words = []
        for k, (a, b) in enumerate(bounds.T):
            a, b = int(a) / 100., int(b) / 100.
            parts = 1 + k % 4
            step = (b - a) / parts
            words.append(alignment_module.Word(f'w{k}', a, b, [
                alignment_module.Phoneme('p', a + j * step,
                                         b if j == parts - 1 else
                                         a + (j + 1) * step)
                for j in range(parts)]))
        texts.append(os.path.join(directory, f'u{index}.TextGrid'))
        waves.append(os.path.join(directory, f'u{index}.wav'))
        alignment_module.Alignment(words).save(texts[-1])
        load.save_wav(waves[-1], audio, 16000)
    return texts, waves


def files_per_second(texts, waves, directory, method, repeats=3):
    emphases_amd.configure(method=method)
    prefixes = [os.path.join(directory, f'{method}_{i}')
                for i in range(len(texts))]
    emphases_amd.from_files_to_files(texts, waves, prefixes, gpu=0)
    best = None
    for _ in range(repeats):
        start = time.perf_counter()
        emphases_amd.from_files_to_files(texts, waves, prefixes, gpu=0)
        torch.cuda.synchronize()
        elapsed = time.perf_counter() - start
        best = elapsed if best is None else min(best, elapsed)
    emphases_amd.configure(method='neural')
    return len(texts) / best


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--files', type=int, default=4096)
    parser.add_argument('--out', default=None)
    arguments = parser.parse_args()
    result = {
        'configs1_pitch_variance': pitch_variance(64, 1000),
        'configs4_pitch_variance': pitch_variance(64, 30000),
    }
    directory = tempfile.mkdtemp()
    try:
        texts, waves = corpus(directory, arguments.files)
        result['files'] = arguments.files
        result['files_per_s_duration_variance'] = files_per_second(
            texts, waves, directory, 'duration-variance')
        result['files_per_s_neural'] = files_per_second(
            texts, waves, directory, 'neural')
    finally:
        shutil.rmtree(directory, ignore_errors=True)
    line = json.dumps(result)
    print(line)
    if arguments.out:
        os.makedirs(arguments.out, exist_ok=True)
        with open(os.path.join(arguments.out, 'baselines_profile.json'),
                  'w') as file:
            file.write(line + '\n')


if __name__ == '__main__':
    main()
