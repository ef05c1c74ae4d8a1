"""`python -m emphases.train` (`emphases/train/__main__.py`): the reference's
flags, with the run's directory in place of the configuration file it is named
after, plus where the data lies and the settings the reference reads from its
configuration - or `--config FILE`, the reference's own way of choosing an
experiment (`config/downsample/sum-input.py` ...), read as data and never
executed."""
import argparse
import ast
import dataclasses
from pathlib import Path

import emphases_amd
from emphases_amd.train import loop


# torch.nn.<Name> of ACTIVATION_FUNCTION -> Config.activation
ACTIVATION_NAMES = {
    'ReLU': 'relu', 'GELU': 'gelu', 'SiLU': 'silu', 'LeakyReLU': 'leaky_relu'}
# names of a configuration file that choose nothing here
IGNORED_NAMES = ('MODULE', 'CONFIG')
# names that are arguments of `train.train`, not fields of `Config`
LOOP_NAMES = {'NUM_STEPS': 'num_steps',
              'MAX_TRAINING_FRAMES': 'max_training_frames'}


def read_config(path):
    """The settings of a reference configuration file
    (`emphases/config/defaults.py` names): ({Config field: value},
    {train.train argument: value}).  The file is parsed with `ast` and never
    executed: only upper-case assignments of literals count, and
    `ACTIVATION_FUNCTION = torch.nn.<Name>`, which is taken by its name; the
    one statement `import torch` that goes with it is skipped.
    ValueError, naming it, for anything else."""
    fields = {field.name for field in dataclasses.fields(emphases_amd.Config)}
    with open(path) as file:
        text = file.read()
    try:
        tree = ast.parse(text, filename=str(path))
    except (SyntaxError, ValueError, MemoryError, RecursionError) as error:
        raise ValueError(
            f'{path} is not a configuration file this trainer can read: '
            f'{error}') from None
    overrides, loop_arguments = {}, {}
    for node in tree.body:
        if isinstance(node, ast.Expr) and \
                isinstance(node.value, ast.Constant) and \
                isinstance(node.value.value, str):
            continue                                    # a docstring
        if isinstance(node, ast.Import) and len(node.names) == 1 and \
                node.names[0].name == 'torch' and \
                node.names[0].asname is None:
            # `import torch`, the first line of the activation experiments
            # (config/hparam-search/gelu.py ...): skipped, never executed
            continue
        if not isinstance(node, ast.Assign) or len(node.targets) != 1 or \
                not isinstance(node.targets[0], ast.Name):
            raise ValueError(
                f'{path}:{node.lineno}: only assignments NAME = literal are '
                'read from a configuration file')
        name = node.targets[0].id
        if name != name.upper():
            raise ValueError(
                f'{path}:{node.lineno}: {name} is not an upper-case setting')
        if name in IGNORED_NAMES:
            continue
        if name == 'ACTIVATION_FUNCTION':
            value = node.value
            if not (isinstance(value, ast.Attribute) and
                    ast.unparse(value.value) == 'torch.nn' and
                    value.attr in ACTIVATION_NAMES):
                raise ValueError(
                    f'{path}:{node.lineno}: ACTIVATION_FUNCTION must be '
                    f'torch.nn.<one of {sorted(ACTIVATION_NAMES)}>, not '
                    f'{ast.unparse(value)}')
            overrides['activation'] = ACTIVATION_NAMES[value.attr]
            continue
        try:
            value = ast.literal_eval(node.value)
        except (ValueError, TypeError, SyntaxError, MemoryError,
                RecursionError):
            raise ValueError(
                f'{path}:{node.lineno}: the value of {name} is not a '
                'literal') from None
        if name in LOOP_NAMES:
            loop_arguments[LOOP_NAMES[name]] = value
        elif name.lower() in fields:
            overrides[name.lower()] = value
        else:
            raise ValueError(
                f'{path}:{node.lineno}: {name} is not a setting this trainer '
                'knows')
    return overrides, loop_arguments


def parse_args(arguments=None):
    parser = argparse.ArgumentParser(description='Train a model')
    parser.add_argument(
        '--config', type=Path,
        help='A configuration file of the reference (upper-case assignments '
             'of literals; parsed, never executed); explicit flags override '
             'it')
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
        '--num_steps', type=int,
        help='The number of updates')
    parser.add_argument(
        '--max_training_frames', type=int,
        help='The frame budget of a padded training batch')
    parser.add_argument(
        '--log_interval', type=int, default=loop.LOG_INTERVAL,
        help='Steps between validations')
    parser.add_argument(
        '--architecture', choices=('convolution', 'transformer'),
        help="The model: 'convolution' (default), or 'transformer', which "
             'trains through TransformerTrainer (downsample_location '
             "'intermediate' or 'loss') or TransformerLocationsTrainer "
             "('input' or 'inference')")
    parser.add_argument(
        '--reference_dropout', action='store_true',
        help="With the transformer: train with the reference's five "
             "dropouts of 0.1 (precision 'f32' only)")
    parser.add_argument(
        '--loss', choices=emphases_amd.config.LOSSES,
        help="The loss: 'bce' (default) or 'mse'")
    parser.add_argument(
        '--downsample_method', choices=emphases_amd.config.DOWNSAMPLE_METHODS,
        help="The word reduction: 'sum' (default), 'average', 'max' or "
             "'center'")
    parser.add_argument(
        '--downsample_location',
        choices=('input', 'intermediate', 'inference', 'loss'),
        help="Where the frames become words: 'intermediate' (default, with "
             "a word decoder), 'inference' (frame-rate loss against "
             "upsampled targets), 'loss' (word-rate loss, no decoder) or, "
             "with the transformer only, 'input' (every word a padded piece "
             'of its own)')
    parser.add_argument(
        '--upsample_method', choices=emphases_amd.config.UPSAMPLE_METHODS,
        help="The interpolation of the targets at --downsample_location "
             "inference: 'linear' (default) or 'nearest'")
    parser.add_argument(
        '--activation', choices=sorted(ACTIVATION_NAMES.values()),
        help="The activation of the conv stacks: 'relu' (default), 'gelu', "
             "'silu' or 'leaky_relu'")
    parser.add_argument(
        '--channels', type=int,
        help='The width of the conv stacks (default 80)')
    parser.add_argument(
        '--layers', type=int,
        help='The layers of each conv stack (default 6)')
    parser.add_argument(
        '--encoder_kernel_size', type=int,
        help='The kernel size of the frame encoder (default 3)')
    parser.add_argument(
        '--decoder_kernel_size', type=int,
        help='The kernel size of the word decoder and the output layer '
             '(default 3)')
    parser.add_argument(
        '--dropout', type=float,
        help='Dropout probability after every activation of the conv stacks '
             '(0 <= p < 1; default: no Dropout modules)')
    parser.add_argument(
        '--precision', choices=emphases_amd.train.PRECISIONS, default='f32',
        help="'f32' (default), or 'bf16x3': the frame-rate convolutions of "
             'the step on the bf16 matrix pipe, two pieces per operand')
    parsed = parser.parse_args(arguments)
    if parsed.downsample_location == 'input' and parsed.config is None and \
            parsed.architecture != 'transformer':
        parser.error("--downsample_location input goes with --architecture "
                     "transformer (the convolution model takes 'input' from "
                     'a --config file)')
    return parsed


def settings(arguments=None):
    """(Config overrides, `train.train` keyword arguments) of a command line:
    the configuration file first, explicit flags over it, the reference's
    defaults for what neither names."""
    arguments = vars(parse_args(arguments))
    path = arguments.pop('config')
    overrides, loop_arguments = ({}, {}) if path is None else \
        read_config(path)
    for name in ('architecture', 'loss', 'downsample_method',
                 'downsample_location',
                 'upsample_method', 'activation', 'channels', 'layers',
                 'encoder_kernel_size', 'decoder_kernel_size', 'dropout'):
        value = arguments.pop(name)
        if value is not None:
            overrides[name] = value
    defaults = {'num_steps': loop.NUM_STEPS,
                'max_training_frames': loop.MAX_TRAINING_FRAMES}
    for name, default in defaults.items():
        if arguments[name] is None:
            arguments[name] = loop_arguments.get(name, default)
    return overrides, arguments


def main(arguments=None):
    overrides, arguments = settings(arguments)
    if overrides:
        emphases_amd.configure(**overrides)
    # (the Transformer is an opt-in of `train.train`: without it the keyword
    # arguments are the ones they always were)
    reference_dropout = arguments.pop('reference_dropout')
    active = emphases_amd.core.active_config()
    if active.architecture == 'transformer':
        # ('intermediate' and 'loss' keep the trainer they always had)
        located = active.downsample_location in ('input', 'inference')
        arguments['trainer'] = \
            emphases_amd.train.TransformerLocationsTrainer if located \
            else emphases_amd.train.TransformerTrainer
        if reference_dropout:
            arguments['trainer_arguments'] = {'reference_dropout': True}
    elif reference_dropout:
        raise SystemExit(
            'error: --reference_dropout goes with the transformer '
            '(--architecture transformer, or ARCHITECTURE in --config)')
    dataset, directory = arguments.pop('dataset'), arguments.pop('directory')
    emphases_amd.train.train(dataset, directory, **arguments)


if __name__ == '__main__':
    main()
