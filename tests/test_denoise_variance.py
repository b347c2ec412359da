"""The variance-guided a-trous denoiser of a progressive render's Color channel on the CPU: rayn_denoise_variance_scratch_bytes, the
VarianceDenoise parameters' validation, and the invariants of the numpy restatement (tests/denoise_variance_np.py) the GPU tests compare
the kernels with: its float32 reading against its float64 one, the closed form of the propagated variance, the inertness of the pixels
that are not guided, and no blur across an edge between two regions the render measured as noise-free."""
import dataclasses

import numpy as np
import pytest

import denoise_variance_np as VN
from denoise_np import H_TAPS
from rayn_amd import film as F


def test_scratch_bytes():
    assert F.denoise_variance_scratch_bytes(1, 1) == 48
    assert F.denoise_variance_scratch_bytes(1280, 720) == 48 * 1280 * 720
    assert F.denoise_variance_scratch_bytes(16384, 16384) == 48 * 16384 * 16384  # 12 GiB: no 32-bit overflow
    assert F.denoise_variance_scratch_bytes((1 << 31) - 1, 1) == 48 * ((1 << 31) - 1)
    # sizes the entry rejects
    assert F.denoise_variance_scratch_bytes(0, 5) == 0 and F.denoise_variance_scratch_bytes(5, 0) == 0
    assert F.denoise_variance_scratch_bytes(1 << 16, 1 << 15) == 0 and F.denoise_variance_scratch_bytes(0xFFFFFFFF, 0xFFFFFFFF) == 0


def test_parameters_are_validated():
    import rayn_amd
    assert rayn_amd.VarianceDenoise is F.VarianceDenoise
    d = F.VarianceDenoise()
    assert 1 <= d.iterations <= 8 and d.sigma_luminance > 0
    with pytest.raises(dataclasses.FrozenInstanceError):
        d.iterations = 3
    for bad in (dict(iterations=0), dict(iterations=9), dict(iterations=2.0), dict(iterations=True), dict(sigma_luminance=-0.5),
                dict(sigma_luminance=float("nan")), dict(sigma_normal=float("inf")), dict(sigma_alpha=-float("inf")),
                dict(sigma_luminance=2.0 ** 31), dict(sigma_normal=1e-10), dict(sigma_alpha="0.1"), dict(sigma_luminance=None)):
        with pytest.raises(ValueError):
            F.VarianceDenoise(**bad)
    for good in (dict(iterations=1), dict(iterations=8), dict(sigma_luminance=0), dict(sigma_normal=0.0, sigma_alpha=0.0),
                 dict(sigma_luminance=2.0 ** 30, sigma_normal=2.0 ** -30), dict(iterations=np.int64(3), sigma_alpha=np.float32(0.25))):
        F.VarianceDenoise(**good)
    # a guide the film lacks (have_mask bit 1 Alpha, bit 3 WorldNormal) is switched off
    assert d.without(15) == d
    assert d.without(15 & ~8) == dataclasses.replace(d, sigma_normal=0.0)
    assert d.without(1) == dataclasses.replace(d, sigma_normal=0.0, sigma_alpha=0.0)


def _film(h, w, seed):
    rng = np.random.default_rng(seed)
    color = rng.uniform(0.0, 1.5, (h * w, 3)).astype(np.float32)
    normal = rng.normal(size=(h * w, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    alpha = (rng.uniform(size=h * w) < 0.7).astype(np.float32)
    return color, alpha, normal


def test_initial_variance_follows_the_tiles():
    """50x37 in 16x16 tiles is the documented under-covered case: 3x2 tiles, x-major, 48x32 pixels."""
    w, h = 50, 37
    color = np.ones((w * h, 3), np.float32)
    m2 = np.full(w * h, 6.0, np.float32)
    epochs = np.array([2, 3, 0, 1, 4, 65536], np.uint32)  # tiles (0,0) (0,1) (1,0) (1,1) (2,0) (2,1) as (tx, ty)
    v = VN.initial_variance(color, m2, epochs, w, h, (16, 16)).reshape(h, w)
    assert np.all(v[:16, :16] == np.float32(3.0)) and np.all(v[16:32, :16] == np.float32(1.0))
    assert np.isnan(v[:32, 16:32]).all()  # n = 0 and n = 1
    assert np.all(v[:16, 32:48] == np.float32(0.5))
    assert np.all(v[16:32, 32:48] == np.float32(6.0) / np.float32(65536 * 65535))
    assert np.isnan(v[32:, :]).all() and np.isnan(v[:, 48:]).all()  # in no tile
    assert np.isfinite(v).sum() == 4 * 256


def test_float32_reading_is_close_to_a_float64_reading(oracle):
    """Initial variances in [1e-4, 1e-1] and sigma_luminance >= 1 keep inv <= 100, where an f32 rounding of a luminance moves e by about
    1e-5.  The colour meets the a-trous restatement's bound (rtol 2e-5, atol 1e-6).  The variance falls by orders of magnitude over the
    passes, so an absolute term would hide it: it is compared relatively alone, at the same rtol."""
    h, w = 24, 31
    color, alpha, normal = _film(h, w, 3)
    v0 = np.random.default_rng(4).uniform(1e-4, 1e-1, h * w).astype(np.float32)
    for L, sigmas in ((1, (4.0, 0.4, 0.3)), (5, (4.0, 0.4, 0.3)), (3, (1.0, 0.0, 0.2)), (2, (2.0, 0.1, 0.0)), (8, (16.0, 0.0, 0.0)), (4, (0.0, 0.4, 0.0))):
        got_c, got_v = VN.atrous(color, alpha, normal, v0, w, h, L, *sigmas)
        want_c, want_v = VN.atrous(color, alpha, normal, v0, w, h, L, *sigmas, dtype=np.float64)
        assert got_c.dtype == got_v.dtype == np.float32 and want_c.dtype == want_v.dtype == np.float64
        rel_v = np.abs(got_v - want_v) / want_v
        print(f"L={L} sigmas={sigmas}: colour max abs {np.abs(got_c - want_c).max():.3g}, variance max rel {rel_v.max():.3g}")
        assert np.allclose(got_c, want_c, rtol=2e-5, atol=1e-6), (L, sigmas, np.abs(got_c - want_c).max())
        assert np.allclose(got_v, want_v, rtol=2e-5, atol=0.0), (L, sigmas, rel_v.max())
        assert not np.array_equal(got_c, color) and not np.array_equal(got_v, v0)  # it did filter


def _dense_closed_form(v0, w, h, L):
    """sum(w^2 v) / (sum w)^2 over the B3 stencil with the taps outside the image dropped, pass by pass, in float64 with explicit loops."""
    v = np.asarray(v0, np.float64).reshape(h, w)
    for i in range(L):
        s = 1 << i
        out = np.zeros_like(v)
        for y in range(h):
            for x in range(w):
                num = den = 0.0
                for ky in range(-2, 3):
                    for kx in range(-2, 3):
                        qy, qx = y + ky * s, x + kx * s
                        if 0 <= qy < h and 0 <= qx < w:
                            wt = H_TAPS[ky + 2] * H_TAPS[kx + 2]
                            num += wt * wt * v[qy, qx]
                            den += wt
                out[y, x] = num / (den * den)
        v = out
    return v.reshape(-1)


def test_variance_has_its_closed_form_when_every_term_is_off(oracle):
    """With the three sigmas 0, e == 0 and w == h h: the weights do not depend on the data.  Relative tolerance 1e-5: about 25 f32
    accumulations per pass at 6e-8 each, three passes, one order of magnitude of room."""
    h, w = 11, 14
    color, alpha, normal = _film(h, w, 5)
    v0 = np.random.default_rng(6).uniform(1e-6, 1.0, h * w).astype(np.float32)
    for L in (1, 3):
        _, got = VN.atrous(color, None, None, v0, w, h, L, 0.0, 0.0, 0.0)
        want = _dense_closed_form(v0, w, h, L)
        assert np.allclose(got, want, rtol=1e-5, atol=0.0), (L, (np.abs(got - want) / want).max())


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_pixels_that_are_not_guided_are_inert(oracle):
    """Tiles with n < 2, under-covered pixels, non-finite colours and negative / non-finite m2 pass through bit for bit, and their values
    do not reach any guided pixel's output."""
    w, h, tile = 50, 37, (16, 16)
    n = w * h
    color, alpha, normal = _film(h, w, 7)
    rng = np.random.default_rng(8)
    m2 = rng.uniform(1e-4, 1e-1, n).astype(np.float32)
    epochs = np.array([2, 5, 0, 1, 64, 3], np.uint32)
    bad_color = rng.choice(n, 40, replace=False)
    color[bad_color[:10], 0] = np.nan
    color[bad_color[10:20], 1] = np.inf
    color[bad_color[20:30], 2] = -np.inf
    color[bad_color[30:], 0] = np.float32(-np.nan)
    bad_m2 = rng.choice(n, 40, replace=False)
    m2[bad_m2] = np.resize(np.array([-1e-3, np.nan, np.inf, -np.inf], np.float32), 40)
    v0 = VN.initial_variance(color, m2, epochs, w, h, tile)
    inert = np.isnan(v0)
    ys, xs = np.divmod(np.arange(n), w)
    assert inert[(ys >= 32) | (xs >= 48)].all() and inert[bad_color].all() and inert[bad_m2].all()
    assert inert[(xs >= 16) & (xs < 32) & (ys < 32)].all()  # the tiles with n = 0 and n = 1
    assert (~inert).sum() > 900
    for L, sigmas in ((1, (4.0, 0.4, 0.3)), (4, (4.0, 0.4, 0.3)), (3, (0.0, 0.0, 0.0))):
        out_c, out_v = VN.denoise(color, alpha, normal, m2, epochs, w, h, tile, L, *sigmas)
        assert np.array_equal(_bits(out_c[inert]), _bits(color[inert])), (L, sigmas)  # payloads and signs included
        assert np.isnan(out_v[inert]).all() and np.isfinite(out_v[~inert]).all() and np.isfinite(out_c[~inert]).all()
        assert not np.array_equal(out_c[~inert], color[~inert])
        # other values in the inert pixels: the guided pixels' outputs keep their bits
        color2, m2_2, alpha2, normal2 = color.copy(), m2.copy(), alpha.copy(), normal.copy()
        finite_inert = inert & np.isfinite(color).all(-1)
        color2[finite_inert] = 1e6
        color2[bad_color] = 123.0  # finite now, but...
        m2_2[bad_color] = np.nan  # ...still not guided
        m2_2[inert & ~np.isin(np.arange(n), bad_color)] = -7.0
        alpha2[inert] = 0.5
        normal2[inert] = 9.0
        assert np.array_equal(np.isnan(VN.initial_variance(color2, m2_2, epochs, w, h, tile)), inert)
        out_c2, out_v2 = VN.denoise(color2, alpha2, normal2, m2_2, epochs, w, h, tile, L, *sigmas)
        assert np.array_equal(_bits(out_c2[~inert]), _bits(out_c[~inert])), (L, sigmas)
        assert np.array_equal(_bits(out_v2[~inert]), _bits(out_v[~inert])), (L, sigmas)


def test_no_blur_across_an_edge_the_render_measured_as_noise_free(oracle):
    """Two regions of one constant colour each (luminances 0.01 apart or more) with m2 == 0 and n >= 2: sqrtf(g_p) == 0, inv == 1e8,
    e >= 1e6 across the edge and dm_expf(-e) == 0.  No output of the first region depends on the second, and S / W over at most 25
    equal-valued terms stays within 25 * 2^-23 relative of the constant."""
    w, h, tile = 32, 32, (16, 16)
    n = w * h
    ys, xs = np.divmod(np.arange(n), w)
    first = (xs + ys // 3) % 32 < 17  # a slanted edge through every tile
    m2 = np.zeros(n, np.float32)
    epochs = np.array([2, 5, 64, 3], np.uint32)
    a_col = np.array([0.30, 0.20, 0.10], np.float32)

    def run(b_col, L):
        color = np.where(first[:, None], a_col, np.asarray(b_col, np.float32)).astype(np.float32)
        lum = lambda c: 0.2126 * float(c[0]) + 0.7152 * float(c[1]) + 0.0722 * float(c[2])
        assert abs(lum(a_col) - lum(b_col)) >= 0.01
        return VN.denoise(color, None, None, m2, epochs, w, h, tile, L, 4.0, 0.0, 0.0)

    for L in (1, 5):
        c1, v1 = run((0.30, 0.22, 0.10), L)  # luminance 0.0143 above the first region's
        c2, v2 = run((5.0, 0.0, 7.0), L)
        assert np.array_equal(_bits(c1[first]), _bits(c2[first])) and np.array_equal(_bits(v1[first]), _bits(v2[first])), L
        assert np.all(np.abs(c1[first] - a_col) <= 25 * 2.0 ** -23 * a_col), L
        assert np.all(np.abs(c2[~first] - np.array([5.0, 0.0, 7.0], np.float32)) <= 25 * 2.0 ** -23 * np.array([5.0, 0.0, 7.0])), L
        assert np.all(v1 == 0) and np.all(v2 == 0)
