"""CPU: bench.py --dump-outputs (bench.dump_outputs): what the last timed step returned, written as float32 .npy files within the
byte budget, whole where it fits and otherwise as a seeded sample that is the same in every run."""
import os

import numpy as np
import torch


def _outs(forwards, pairs, B, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    return [([torch.randn(B, 2, 8 * h, 8 * w, generator=g) for _ in range(pairs)],
             [torch.randn(B, 2, h, w, generator=g) for _ in range(pairs)]) for _ in range(forwards)]


def test_dump_outputs_whole_and_sampled(tmp_path):
    import bench
    outs = _outs(2, 3, 2, 6, 10, seed=1)            # up: 2 x 2 x 2 x 48 x 80 = 30720 elements per pair; low: 480
    budget = 4 * (3 * 480 + 3 * 10000)
    names = bench.dump_outputs(outs, str(tmp_path / "a"), budget_bytes=budget)
    assert sorted(names) == sorted([f"flow_{k}_{i}" for k in ("up", "low") for i in range(3)])
    total = 0
    for i in range(3):
        low = np.load(tmp_path / "a" / f"flow_low_{i}.npy")
        assert low.dtype == np.float32
        np.testing.assert_array_equal(low, torch.cat([o[1][i] for o in outs]).numpy())           # small: written whole
        up = np.load(tmp_path / "a" / f"flow_up_{i}.npy")
        full = torch.cat([o[0][i] for o in outs]).reshape(-1).numpy()
        assert up.dtype == np.float32 and up.ndim == 1 and up.size == 10000
        idx = torch.randperm(full.size, generator=torch.Generator().manual_seed(0))[:up.size].sort().values.numpy()
        np.testing.assert_array_equal(up, full[idx])                                             # large: the seeded sample
        total += low.nbytes + up.nbytes
    assert total <= budget
    bench.dump_outputs(outs, str(tmp_path / "b"), budget_bytes=budget)
    for n in names:                                                                              # same arguments, same files
        assert (tmp_path / "a" / (n + ".npy")).read_bytes() == (tmp_path / "b" / (n + ".npy")).read_bytes()


def test_dump_outputs_headline_shape_fits_64_mb(tmp_path):
    """The default workload (8 clips, 440 x 1024, 3 pairs: 87 MB of upsampled flows) stays under 64 MB on disk."""
    import bench
    outs = [([torch.zeros(8, 2, 440, 1024) for _ in range(3)], [torch.zeros(8, 2, 55, 128) for _ in range(3)])]
    names = bench.dump_outputs(outs, str(tmp_path))
    assert len(names) == 6
    assert sum(os.path.getsize(tmp_path / (n + ".npy")) for n in names) <= 64_000_000
