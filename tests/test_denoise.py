"""The a-trous denoiser of the Color channel on the CPU: rayn_denoise_scratch_bytes, the Denoise parameters' validation, and the
invariants of the numpy restatement (tests/denoise_np.py) the GPU tests compare the kernel with."""
import dataclasses

import numpy as np
import pytest

import denoise_np
from rayn_amd import film as F


def test_scratch_bytes():
    assert F.denoise_scratch_bytes(1, 1) == 48
    assert F.denoise_scratch_bytes(1280, 720) == 48 * 1280 * 720
    assert F.denoise_scratch_bytes(16384, 16384) == 48 * 16384 * 16384  # 12 GiB: no 32-bit overflow
    assert F.denoise_scratch_bytes((1 << 31) - 1, 1) == 48 * ((1 << 31) - 1)
    # sizes the entry rejects
    assert F.denoise_scratch_bytes(0, 5) == 0 and F.denoise_scratch_bytes(5, 0) == 0
    assert F.denoise_scratch_bytes(1 << 16, 1 << 15) == 0 and F.denoise_scratch_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0


def test_denoise_parameters_are_validated():
    d = F.Denoise()
    assert (d.iterations, d.sigma_color, d.sigma_normal, d.sigma_alpha) == (5, 0.5, 0.4, 0.3)
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.iterations = 3
    for bad in (dict(iterations=0), dict(iterations=9), dict(iterations=2.0), dict(iterations=True), dict(sigma_color=-0.5),
                dict(sigma_color=float("nan")), dict(sigma_normal=float("inf")), dict(sigma_alpha=-float("inf")), dict(sigma_color=2.0 ** 31),
                dict(sigma_normal=1e-10), dict(sigma_alpha="0.1"), dict(sigma_color=None)):
        with pytest.raises(ValueError):
            F.Denoise(**bad)
    for good in (dict(iterations=1), dict(iterations=8), dict(sigma_color=0), dict(sigma_normal=0.0, sigma_alpha=0.0),
                 dict(sigma_color=2.0 ** 30, sigma_normal=2.0 ** -30), dict(iterations=np.int64(3), sigma_alpha=np.float32(0.25))):
        F.Denoise(**good)
    # a guide the film lacks (have_mask bit 1 Alpha, bit 3 WorldNormal) is switched off
    assert d.without(15) == d
    assert d.without(15 & ~8) == F.Denoise(sigma_normal=0.0)
    assert d.without(1) == F.Denoise(sigma_normal=0.0, sigma_alpha=0.0)


def _film(h, w, seed):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 1.5, (h * w, 3)).astype(np.float32)
    normal = rng.normal(size=(h * w, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    alpha = (rng.uniform(size=h * w) < 0.7).astype(np.float32)
    return color, alpha, normal


def test_non_finite_centres_pass_through(oracle):
    color, alpha, normal = _film(9, 11, 1)
    specials = np.array([np.nan, np.inf, -np.inf, np.float32(-np.nan)], np.float32)
    at = [0, 17, 50, 98]
    for i, v in zip(at, specials):
        color[i, i % 3] = v
    bits = color.view(np.uint32).copy()
    for sigmas in ((0.5, 0.4, 0.3), (0.0, 0.0, 0.0), (1.0, 0.0, 0.0)):
        out = denoise_np.atrous(color, alpha, normal, 11, 9, 3, *sigmas)
        assert np.array_equal(out[at].view(np.uint32), bits[at]), sigmas  # payloads and signs included
        others = np.setdiff1d(np.arange(99), at)
        assert np.all(np.isfinite(out[others]))  # the non-finite taps were skipped by every other pixel
    assert np.array_equal(color.view(np.uint32), bits)  # the input is not modified


def test_constant_image_stays_constant(oracle):
    h, w = 13, 17
    for value in (0.0, 0.3, 1.0, 7.25, 1e-30, 3e30):
        color = np.full((h * w, 3), value, np.float32)
        _, alpha, normal = _film(h, w, 2)
        for sigmas in ((0.5, 0.4, 0.3), (0.0, 0.0, 0.0), (2.0 ** -30, 0.0, 0.0)):
            for L in (1, 4):
                out = denoise_np.atrous(color, alpha, normal, w, h, L, *sigmas)
                # (w c) / w rounds: a few ulp per pass, not exact
                ulp = np.abs(out.view(np.int32).astype(np.int64) - color.view(np.int32).astype(np.int64))
                assert ulp.max() <= 8 * L, (value, sigmas, L, ulp.max())


def test_float32_reading_is_close_to_a_float64_reading(oracle):
    color, alpha, normal = _film(24, 31, 3)
    for L, sigmas in ((1, (0.5, 0.4, 0.3)), (5, (0.5, 0.4, 0.3)), (3, (1.0, 0.0, 0.2)), (2, (0.0, 0.1, 0.0)), (8, (4.0, 0.0, 0.0))):
        got = denoise_np.atrous(color, alpha, normal, 31, 24, L, *sigmas)
        want = denoise_np.atrous(color, alpha, normal, 31, 24, L, *sigmas, dtype=np.float64)
        assert got.dtype == np.float32 and want.dtype == np.float64
        assert np.allclose(got, want, rtol=2e-5, atol=1e-6), (L, sigmas, np.abs(got - want).max())
        assert not np.array_equal(got, color)  # it did filter
