"""bench.py --dump-outputs on the CPU: the film channels a timed step returned, written as float32 .npy files, within the 64 MB limit
(a larger film as one fixed, seeded pixel sample)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def _film(n, seed):
    g = torch.Generator().manual_seed(seed)
    return {"color": torch.rand(n, 3, generator=g), "alpha": torch.rand(n, generator=g), "background": torch.rand(n, 3, generator=g),
            "normal": torch.rand(n, 3, generator=g)}


def test_small_film_is_written_whole(tmp_path):
    film = _film(64 * 48, 1)
    rec = bench.dump_outputs(str(tmp_path), film)
    assert rec["sampled_pixels"] is None and rec["pixels"] == 64 * 48
    assert sorted(os.listdir(tmp_path)) == ["alpha.npy", "background.npy", "color.npy", "normal.npy"]
    for k, v in film.items():
        a = np.load(tmp_path / f"{k}.npy")
        assert a.dtype == np.float32 and np.array_equal(a, v.numpy()), k
        assert rec["arrays"][k] == list(v.shape)


def test_large_film_is_a_fixed_sample_within_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 1 << 16)
    n = 10000  # 400 000 bytes of film
    film = _film(n, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    rec = bench.dump_outputs(str(a), film)
    bench.dump_outputs(str(b), _film(n, 3))
    m = rec["sampled_pixels"]
    assert 0 < m < n and rec["arrays"]["pixel_index"] == [m]
    assert sum(os.path.getsize(a / f) for f in os.listdir(a)) <= 1 << 16
    idx = np.load(a / "pixel_index.npy")
    assert idx.dtype == np.float64 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(idx, np.load(b / "pixel_index.npy"))  # the same pixels whatever the film holds
    for k, v in film.items():
        got = np.load(a / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v.numpy()[idx.astype(np.int64)]), k
