"""CPU: `bench.py --dump-outputs DIR` writes what the last timed step returned as float32 .npy files, within its size budget, and the
sample it keeps of larger outputs is the same in every run."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _gathered(seed):
    g = torch.Generator().manual_seed(seed)
    return {"tokens": torch.randint(3, 152064, (1, 2, 12), generator=g, dtype=torch.int32),
            "out": torch.randint(0, 256, (1, 2, 3, 64, 64), generator=g).to(torch.uint8),
            "count": torch.tensor([2], dtype=torch.int32)}


def test_dump_writes_every_output_in_float32(tmp_path):
    bench = _bench()
    g = _gathered(0)
    bench.dump_outputs(g, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["image.npy", "tokens.npy"]          # the gather's row count is bookkeeping, not an output
    for name, key in (("tokens", "tokens"), ("image", "out")):
        a = np.load(tmp_path / f"{name}.npy")
        assert a.dtype == np.float32 and a.shape == tuple(g[key].shape)
        assert np.array_equal(a, g[key].numpy().astype(np.float64))           # token ids and pixels are exact in float32


def test_dump_of_large_outputs_is_a_fixed_sample_within_budget(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BYTES", 4096 * 2 + 20000)
    g = _gathered(1)
    runs = []
    for k in range(2):
        d = tmp_path / str(k)
        bench.dump_outputs(g, str(d))
        runs.append({n: np.load(d / f"{n}.npy") for n in ("tokens", "image")})
        assert sum(os.path.getsize(d / f) for f in os.listdir(d)) <= bench.DUMP_BYTES
    for n, key in (("tokens", "tokens"), ("image", "out")):
        a = runs[0][n]
        assert a.ndim == 1 and 0 < a.size < g[key].numel() and np.array_equal(a, runs[1][n])
        assert np.isin(a, g[key].numpy().reshape(-1)).all()
