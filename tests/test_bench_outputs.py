"""bench.py --dump-outputs / --full: the arrays are written as float32 .npy within the size cap, a larger one as the same seeded sample
every time; the side measurements are off unless --full asks for them."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_dump_outputs_writes_float32_and_samples_large_arrays_the_same_way(tmp_path):
    small = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    big = torch.randn(bench.DUMP_MAX_ELEMS + 12345, generator=torch.Generator().manual_seed(5))
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), {"small": small, "big": big, "scalars": torch.tensor([0.5, 0.25, 0.125], dtype=torch.float64)})
    a_small, a_big = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "big.npy")
    assert a_small.dtype == np.float32 and a_small.shape == (2, 3, 4) and np.array_equal(a_small, small.numpy())
    assert np.load(tmp_path / "a" / "scalars.npy").dtype == np.float32
    assert a_big.dtype == np.float32 and a_big.shape == (bench.DUMP_MAX_ELEMS,)
    assert np.array_equal(a_big, np.load(tmp_path / "b" / "big.npy"))                  # the same positions in every run
    assert np.isin(a_big[:1000], big.numpy()).all()                                      # ... taken from the array itself
    # three arrays at the cap (logits, probabilities, weights) stay under 64 MB on disk
    assert 3 * os.path.getsize(tmp_path / "a" / "big.npy") < 64e6


def test_full_and_dump_outputs_are_off_by_default():
    plain = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert not plain.full and plain.dump_outputs is None and plain.steps == 7 and plain.warmup == 2
    full = bench.parse(["--gpus", "1", "--steps", "7", "--warmup", "2", "--full", "--dump-outputs", "out"])
    assert full.full and full.dump_outputs == "out"
