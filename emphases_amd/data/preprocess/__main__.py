"""`python -m emphases.data.preprocess` (`emphases/data/preprocess/
__main__.py`): the reference's flags, plus where the cache lies and which
features to write."""
import argparse
from pathlib import Path

from . import core


def parse_args(arguments=None):
    parser = argparse.ArgumentParser(
        description='Write the feature cache of datasets')
    parser.add_argument(
        '--datasets', nargs='+', default=['libritts'],
        help='The datasets to preprocess')
    parser.add_argument(
        '--gpu', type=int,
        help='The index of the GPU to compute on')
    # (additions: the reference reads the cache directory from its
    # configuration and always writes every feature)
    parser.add_argument(
        '--cache_dir', type=Path, required=True,
        help='The dataset cache (<dataset>/**/*.wav in; <dataset>/mels, '
             'loudness, pitch out)')
    parser.add_argument(
        '--features', nargs='+', choices=core.FEATURES,
        help='The features to write (default: mels and loudness, and pitch '
             'when the penn tracker is installed)')
    parser.add_argument(
        '--files_per_batch', type=int, default=256,
        help='Files per batch on the GPU')
    return parser.parse_known_args(arguments)[0]


def main(arguments=None):
    core.datasets(**vars(parse_args(arguments)))


if __name__ == '__main__':
    main()
