"""python -m vlrlhf.eval.merge_shards <output_path> N: joins <output_path>.shard0 .. .shard<N-1> (written by an entry point run with
--num_shards N --shard_id i) in order and scores them as the single run would: the result lands at <output_path>."""
import sys
from importlib import import_module

from .utils import read_shards


def merge(output_path, num_shards):
    benchmark, rows = read_shards(output_path, num_shards)
    print(f"[{benchmark}] {len(rows)} rows from {num_shards} shards")
    return import_module(f"vlrlhf.eval.{benchmark}").finalize(rows, output_path)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 2:
        raise SystemExit("usage: python -m vlrlhf.eval.merge_shards <output_path> <num_shards>")
    return merge(argv[0], int(argv[1]))


if __name__ == "__main__":
    main()
