"""bench.py --dump-outputs (no GPU): the files stay inside the 64 MB budget, keep float32 / float64, and a sampled array holds the
same elements in every run."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import bench


def _arrays():
    g = torch.Generator().manual_seed(5)
    out = [("grad_%02d" % k, torch.randn(1 << 20, generator=g)) for k in range(26)]
    out += [("color", torch.randn(3, 40, 60, generator=g)), ("radii", torch.randint(0, 9, (500,), generator=g, dtype=torch.int32)),
            ("wide", torch.randn(1000, generator=g, dtype=torch.float64)), ("missing", None)]
    return out


def test_dump_stays_in_budget_and_keeps_small_arrays_whole(tmp_path):
    arrays = _arrays()
    info = bench.dump_outputs(str(tmp_path), arrays)
    files = sorted(os.listdir(tmp_path))
    assert files == sorted(n + ".npy" for n, t in arrays if t is not None) and set(info) == {f[:-4] for f in files}
    assert sum(os.path.getsize(os.path.join(tmp_path, f)) for f in files) <= 64 << 20
    color = np.load(os.path.join(tmp_path, "color.npy"))
    assert color.dtype == np.float32 and np.array_equal(color, dict(arrays)["color"].numpy().reshape(-1))
    radii = np.load(os.path.join(tmp_path, "radii.npy"))
    assert radii.dtype == np.float32 and np.array_equal(radii, dict(arrays)["radii"].numpy().astype(np.float32))
    assert np.load(os.path.join(tmp_path, "wide.npy")).dtype == np.float64
    big = np.load(os.path.join(tmp_path, "grad_00.npy"))
    assert info["grad_00"]["sampled"] and 0 < big.size < (1 << 20) and big.dtype == np.float32
    assert np.isin(big, dict(arrays)["grad_00"].numpy()).all()


def test_dump_sample_is_the_same_in_every_run(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), _arrays())
    bench.dump_outputs(str(b), _arrays())
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
