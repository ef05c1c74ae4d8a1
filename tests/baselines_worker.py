"""One rank of a two-process run of a baseline through
`emphases_amd.dist.from_files_to_files` (started by
tests/test_gpu_baselines.py as a fresh child process; never imported by
pytest).

    python tests/baselines_worker.py <method> <out.pt> <text files ...> -- \
        <audio files ...> -- <output prefixes ...>

Reads RANK / WORLD_SIZE / MASTER_ADDR / MASTER_PORT like a torchrun worker,
joins a gloo group and saves the gathered scores.
"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402


def main():
    method, out = sys.argv[1:3]
    rest = sys.argv[3:]
    cut = rest.index('--')
    texts, rest = rest[:cut], rest[cut + 1:]
    cut = rest.index('--')
    audios, prefixes = rest[:cut], rest[cut + 1:]
    import emphases_amd
    from emphases_amd import dist
    torch.distributed.init_process_group(
        'gloo', rank=int(os.environ['RANK']),
        world_size=int(os.environ['WORLD_SIZE']))
    try:
        scores = dist.from_files_to_files(
            texts, audios, prefixes, config=emphases_amd.Config(method=method))
        torch.save([s.cpu() for s in scores], out)
    finally:
        torch.distributed.destroy_process_group()


if __name__ == '__main__':
    main()
