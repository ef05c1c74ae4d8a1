"""`python -m emphases.evaluate` (`emphases/evaluate/__main__.py`): the
reference's flags, plus where the data lies and what to evaluate."""
import argparse
from pathlib import Path

import emphases_amd


def parse_args():
    parser = argparse.ArgumentParser(
        description='Evaluate emphasis annotation on annotated datasets')
    parser.add_argument(
        '--datasets', nargs='+', default=['libritts'],
        help='The datasets to evaluate')
    parser.add_argument(
        '--checkpoint', type=Path,
        help='The checkpoint file to evaluate')
    parser.add_argument(
        '--gpu', type=int,
        help='The index of the GPU to use for evaluation')
    # (additions: the reference reads these from its configuration)
    parser.add_argument(
        '--partition_dir', type=Path, required=True,
        help='The directory of the partition files (<dataset>.json)')
    parser.add_argument(
        '--cache_dir', type=Path, default=Path('data/cache'),
        help='The dataset cache (<dataset>/audio, alignment, scores)')
    parser.add_argument(
        '--eval_dir', type=Path, default=Path('eval'),
        help='Where <name>/overall.json and granular.json are written')
    parser.add_argument(
        '--name', default='emphases',
        help='The name of the evaluation (its directory under --eval_dir)')
    parser.add_argument(
        '--method', choices=emphases_amd.config.METHODS,
        help="the emphasis annotation method: 'neural' (default, the model) "
             'or a baseline')
    parser.add_argument(
        '--precision', default='f32',
        choices=sorted(emphases_amd.engine.PRECISIONS),
        help='f32 (default), or an opt-in precision of the model')
    return parser.parse_args()


def main():
    arguments = vars(parse_args())
    method = arguments.pop('method')
    if method is not None:
        emphases_amd.configure(method=method)
    emphases_amd.evaluate.datasets(**arguments)


if __name__ == '__main__':
    main()
