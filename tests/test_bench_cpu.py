"""bench.dump_outputs (`bench.py --dump-outputs DIR`) on CPU tensors: dtypes, shapes, and the fixed sample of a large output."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float_arrays_and_a_fixed_sample_of_large_ones(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 1000)
    g = torch.Generator().manual_seed(5)
    big, small = torch.randn(7, 900, generator=g), torch.randn(2, 3, 4, generator=g)
    cm = torch.randint(0, 1 << 30, (25, 25), dtype=torch.int32, generator=g)
    arrays = {"big": big, "small": small, "cm": cm, "loss": torch.tensor([0.25]), "f64": torch.randn(3, dtype=torch.float64, generator=g)}
    written = bench.dump_outputs(str(tmp_path / "a"), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in arrays}
    assert written == {n: v.nbytes for n, v in a.items()}
    # small arrays keep their shape; integer counts become exact float64, floating point stays in its precision
    assert a["small"].dtype == np.float32 and np.array_equal(a["small"], small.numpy())
    assert a["cm"].dtype == np.float64 and np.array_equal(a["cm"], cm.numpy().astype(np.float64))
    assert a["f64"].dtype == np.float64 and a["loss"].shape == (1,) and a["loss"][0] == np.float32(0.25)
    # a large array: DUMP_SAMPLE of its elements, at sorted positions that depend on its size alone
    assert a["big"].shape == (1000,) and a["big"].dtype == np.float32
    flat = big.reshape(-1).numpy()
    # the positions, read back through a tensor that holds its own index, are the same for another tensor of that size
    bench.dump_outputs(str(tmp_path / "b"), {"big": big + 1.0, "iota": torch.arange(big.numel(), dtype=torch.float32)})
    idx = np.load(tmp_path / "b" / "iota.npy").astype(np.int64)
    assert (np.diff(idx) >= 0).all() and idx.min() >= 0 and idx.max() < big.numel()
    assert np.array_equal(a["big"], flat[idx]) and np.array_equal(np.load(tmp_path / "b" / "big.npy"), (big + 1.0).reshape(-1).numpy()[idx])
