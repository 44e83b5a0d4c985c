"""bench.py --dump-outputs: what is written, and that the sample of a large output is the same in every run."""
import os

import numpy as np
import torch

import bench


def test_a_small_output_is_written_whole():
    f = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    out = bench.output_sample(f, limit=24)
    assert out.dtype == np.float32 and np.array_equal(out, f.reshape(-1).numpy())


def test_a_large_output_is_a_fixed_sorted_sample_within_the_limit():
    f = torch.arange(100_000, dtype=torch.float64).reshape(4, 25_000)
    a, b = bench.output_sample(f, limit=1000), bench.output_sample(f.clone(), limit=1000)
    assert a.dtype == np.float64 and a.size == 1000
    assert np.array_equal(a, b)                                   # same positions in every run
    assert (np.diff(a) >= 0).all()                                # in ascending order of position
    assert bench.DUMP_VALUES * 8 <= 64 << 20                      # at most 64 MB even in fp64


def test_outputs_are_written_as_npy_files(tmp_path):
    bench.write_outputs(str(tmp_path / "out"), {"f": np.ones(5, np.float32)})
    assert np.array_equal(np.load(os.path.join(tmp_path, "out", "f.npy")), np.ones(5, np.float32))


def test_the_plain_run_and_full_are_options():
    args = bench.parse(["--steps", "7"])
    assert args.steps == 7 and not args.full and args.dump_outputs is None and bench.timed_batches(args) == 1
    args = bench.parse(["--full", "--dump-outputs", "d"])
    assert args.full and args.dump_outputs == "d" and bench.timed_batches(args) == 5
    assert bench.timed_batches(bench.parse(["--batches", "3"])) == 3
