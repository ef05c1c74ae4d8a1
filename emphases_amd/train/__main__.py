"""`python -m emphases.train` (`emphases/train/__main__.py`): the reference's
flags, with the run's directory in place of the configuration file it is named
after, plus where the data lies and the settings the reference reads from its
configuration."""
import argparse
from pathlib import Path

import emphases_amd
from emphases_amd.train import loop


def parse_args(arguments=None):
    parser = argparse.ArgumentParser(description='Train a model')
    parser.add_argument(
        '--dataset', default='libritts',
        help='The dataset to train on')
    parser.add_argument(
        '--gpu', type=int,
        help='The gpu to run training on')
    parser.add_argument(
        '--directory', type=Path, required=True,
        help='Where checkpoints and scalars.jsonl are written; a run resumes '
             'from the latest checkpoint found there')
    parser.add_argument(
        '--partition_dir', type=Path, required=True,
        help='The directory of the partition files (<dataset>.json)')
    parser.add_argument(
        '--cache_dir', type=Path, default=Path('data/cache'),
        help='The dataset cache (<dataset>/mels, scores, alignment, ...)')
    parser.add_argument(
        '--num_steps', type=int, default=loop.NUM_STEPS,
        help='The number of updates')
    parser.add_argument(
        '--max_training_frames', type=int, default=loop.MAX_TRAINING_FRAMES,
        help='The frame budget of a padded training batch')
    parser.add_argument(
        '--log_interval', type=int, default=loop.LOG_INTERVAL,
        help='Steps between validations')
    parser.add_argument(
        '--loss', choices=emphases_amd.config.LOSSES,
        help="The loss: 'bce' (default) or 'mse'")
    parser.add_argument(
        '--downsample_method', choices=emphases_amd.config.DOWNSAMPLE_METHODS,
        help="The word reduction: 'sum' (default), 'average', 'max' or "
             "'center' (the last two at --downsample_location inference or "
             'loss only)')
    parser.add_argument(
        '--downsample_location',
        choices=('intermediate', 'inference', 'loss'),
        help="Where the frames become words: 'intermediate' (default, with "
             "a word decoder), 'inference' (frame-rate loss against "
             "upsampled targets) or 'loss' (word-rate loss, no decoder)")
    parser.add_argument(
        '--upsample_method', choices=emphases_amd.config.UPSAMPLE_METHODS,
        help="The interpolation of the targets at --downsample_location "
             "inference: 'linear' (default) or 'nearest'")
    parser.add_argument(
        '--dropout', type=float,
        help='Dropout probability after every activation of the conv stacks '
             '(0 <= p < 1; default: no Dropout modules)')
    parser.add_argument(
        '--precision', choices=emphases_amd.train.PRECISIONS, default='f32',
        help="'f32' (default), or 'bf16x3': the frame-rate convolutions of "
             'the step on the bf16 matrix pipe, two pieces per operand')
    return parser.parse_args(arguments)


def main(arguments=None):
    arguments = vars(parse_args(arguments))
    overrides = {
        name: arguments.pop(name)
        for name in ('loss', 'downsample_method', 'downsample_location',
                     'upsample_method', 'dropout')}
    overrides = {
        name: value for name, value in overrides.items() if value is not None}
    if overrides:
        emphases_amd.configure(**overrides)
    dataset, directory = arguments.pop('dataset'), arguments.pop('directory')
    emphases_amd.train.train(dataset, directory, **arguments)


if __name__ == '__main__':
    main()
