"""The HDR display transform (include/rayn_hip.h: rayn_hip_display_pixels_device) on the host: its numpy restatement tests/display_np.py
against image.color_image (identity parameters), against its own float64 reading, and on inputs whose answer is known; Display's
validation, the ABI struct and the PFM writer.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_np as D
import rayn_amd as R
from display_cases import film
from rayn_amd import _abi, _lib, image
from rayn_amd.film import Bloom, Display

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
def params(tone="linear", exposure=0.0, bloom=None, key=0.18, white=4.0, adapt=1.0):
    return Display(exposure=exposure, key=key, tone=tone, white=white, bloom=bloom).to_abi(adapt)


ARMS = [("rgba", True, True, True), ("color_bg", False, True, False), ("color_only", False, False, False)]


@pytest.mark.parametrize("name,transparent,with_bg,with_alpha", ARMS)
@pytest.mark.parametrize("size", [(1, 1), (17, 13), (33, 65)])
def test_identity_parameters_reproduce_color_image(name, transparent, with_bg, with_alpha, size):
    w, h = size
    color, background, alpha = film(w, h, 7 + w, with_background=with_bg, with_alpha=with_alpha)
    got = D.display(color, w, h, params(), background, alpha, transparent)
    want = image.color_image(color.reshape(h, w, 3), None if background is None else background.reshape(h, w, 3),
                             None if alpha is None else alpha.reshape(h, w), transparent)
    assert got["image"].dtype == np.uint8 and got["image"].shape == want.shape
    assert np.array_equal(got["image"], want)
    c = D.input_color(color, background, transparent)
    assert np.array_equal(np.isnan(got["d"]), np.isnan(c))
    assert np.array_equal(got["d"][~np.isnan(c)].view(np.uint32), c[~np.isnan(c)].view(np.uint32))  # d has the bits of c


# Largest |d32 - d64| / max(|d64|, 1e-3 * mean |d64|) over the cases below, measured here: 1.44e-6 (reinhard, auto exposure, bloom of 1
# level at 33x65: e * c - threshold cancels next to the threshold; without bloom the largest is 3.0e-7).  The bound is 8x that; a wrong
# constant, tap or weight is off by 1e-2 or more.
F64_TOLERANCE = 1.2e-5


@pytest.mark.parametrize("tone", ["linear", "reinhard", "aces"])
@pytest.mark.parametrize("exposure", ["auto", 1.5])
@pytest.mark.parametrize("levels", [0, 1, 3, 8])
def test_float32_reading_agrees_with_float64(tone, exposure, levels):
    w, h = 33, 65
    color, background, _ = film(w, h, 11, adversarial=False)
    p = params(tone, exposure, Bloom(0.8, 0.6, levels) if levels else None)
    a = D.display(color, w, h, p, background)
    b = D.display(color, w, h, p, background, dtype=np.float64)
    d32, d64 = a["d"].astype(np.float64), b["d"]
    err = np.abs(d32 - d64) / np.maximum(np.abs(d64), 1e-3 * np.abs(d64).mean())
    print(f"{tone} {exposure} {levels}: max rel err {err.max():.3e}, e32 {a['e']:.9g} e64 {b['e']:.9g}")
    assert err.max() <= F64_TOLERANCE
    assert abs(float(a["e"]) - float(b["e"])) <= F64_TOLERANCE * float(b["e"])
    if levels:
        assert np.allclose(a["bloom"], b["bloom"], rtol=F64_TOLERANCE, atol=F64_TOLERANCE * np.abs(b["bloom"]).mean())


# 32 x 16 = 512 pixels = two full blocks, so every sum of the tree adds equal values and is exact: m is logf of the luminance itself.
# The grey levels are powers of two near 1, where |m| <= 0.7 and the rounding of m (half an ulp of m) moves expf(m) by less than half an
# ulp; with the roundings of expf and of the division that stays within the 1 ulp asked for.
@pytest.mark.parametrize("grey", [0.5, 1.0, 2.0])
def test_metering_of_a_constant_image(grey):
    w, h, key = 32, 16, np.float32(0.18)
    color = np.full((w * h, 3), grey, np.float32)
    got = D.display(color, w, h, params(exposure="auto", key=0.18))
    c64 = color[0].astype(np.float64)
    l64 = (np.float64(np.float32(0.2126)) * c64[0] + np.float64(np.float32(0.7152)) * c64[1]) + np.float64(np.float32(0.0722)) * c64[2]
    want = np.float64(key) / l64
    ulp = np.spacing(np.float32(want))
    assert abs(np.float64(got["e"]) - want) <= ulp, (got["e"], want)
    assert got["state"][1] == 1 and np.float32(got["state"][0]) == np.float32(got["m"])


@pytest.mark.parametrize("fill", [0.0, np.nan, -2.0, np.inf])
def test_nothing_to_meter_gives_unit_exposure_and_keeps_the_state(fill):
    w, h = 17, 13
    color = np.full((w * h, 3), fill, np.float32)
    for state in ((0.0, 0), (np.float32(-1.25), 1)):
        got = D.display(color, w, h, params(exposure="auto", adapt=0.25), state=state)
        assert got["e"] == np.float32(1.0)
        assert got["state"] == state


def test_adaptation_blends_the_metered_value():
    w, h = 32, 16
    dark, light = np.full((w * h, 3), 0.5, np.float32), np.full((w * h, 3), 2.0, np.float32)
    first = D.display(dark, w, h, params(exposure="auto", adapt=0.25))  # a fresh state takes its own value whatever adapt is
    assert first["state"][0] == D.display(dark, w, h, params(exposure="auto", adapt=1.0))["state"][0]
    second = D.display(light, w, h, params(exposure="auto", adapt=0.25), state=first["state"])
    m0, m1 = first["state"][0], D.display(light, w, h, params(exposure="auto"))["state"][0]
    assert second["state"][0] == np.float32(m0 + np.float32(np.float32(m1 - m0) * np.float32(0.25)))
    assert m0 < second["state"][0] < m1


def test_bloom_of_one_bright_pixel_is_non_negative_and_symmetric():
    w = h = 16
    f = np.float32

    def plane(x, y):
        c = np.zeros((h, w, 3), f)
        c[y, x] = (50.0, 20.0, 5.0)
        return D.bloom(c.reshape(-1, 3), f(1.0), w, h, 4, 1.0, 0.5).reshape(h, w, 3)

    b = plane(5, 9)
    assert np.isfinite(b).all() and (b >= 0).all() and b[9, 5].min() > 0 and b.max() == b[9, 5].max()
    # mirrored input, mirrored bloom - bit for bit: pairs map to pairs in a power-of-two image, and every sum only swaps its operands
    assert np.array_equal(plane(w - 1 - 5, 9), b[:, ::-1])
    assert np.array_equal(plane(5, h - 1 - 9), b[::-1])
    # a pixel on the diagonal: the transposed plane regroups the sums ((A + B) + (C + D) becomes (A + C) + (B + D)), so to rounding only
    t = plane(6, 6)
    assert np.allclose(t, t.transpose(1, 0, 2), rtol=1e-5, atol=0)


@pytest.mark.parametrize("size", [(1, 1), (3, 2), (1, 7)])
def test_bloom_with_more_levels_than_the_pyramid_is_deep(size):
    w, h = size
    assert D.level_sizes(w, h, 8)[-1] == (1, 1) and D.level_sizes(w, h, 8)[4] == (1, 1)
    color, _, _ = film(w, h, 3, adversarial=False, with_background=False, with_alpha=False)
    color *= 40
    b32 = D.bloom(color, np.float32(1.0), w, h, 8, 0.5, 0.7)
    b64 = D.bloom(color.astype(np.float64), np.float64(1.0), w, h, 8, 0.5, 0.7, np.float64)
    assert b32.shape == (w * h, 3) and np.isfinite(b32).all() and (b32 >= 0).all() and b32.max() > 0
    assert np.allclose(b32, b64, rtol=F64_TOLERANCE)


def test_scratch_bytes():
    _lib.build()
    nb = (300 * 220 + 255) // 256
    want = 256 + (8 * nb + 255) // 256 * 256 + 16 * sum(w * h for w, h in D.level_sizes(300, 220, 3)[1:])
    assert R.film.display_scratch_bytes(300, 220, 3) == want
    assert R.film.display_scratch_bytes(300, 220, 0) == 256 + (8 * nb + 255) // 256 * 256
    assert R.film.display_scratch_bytes(0, 220, 3) == 0 and R.film.display_scratch_bytes(300, 220, 9) == 0
    assert R.film.display_scratch_bytes(1 << 16, 1 << 15, 0) == 0


def test_display_validation():
    d = Display()
    assert d.auto and d.levels == 0 and d.tone == "aces" and d.adapt(1.0) == 1.0
    assert Display(exposure=0.0, tone="linear").to_abi().exposure_scale == 1.0 and Display(exposure=-1).to_abi().exposure_scale == 0.5
    assert Display(bloom=Bloom()).levels == 5 and Display(white=2.0).to_abi().iw2 == 0.25
    a = Display(adaptation=0.5).adapt(1.0 / 24.0)
    assert a == float(np.float32(1.0 - np.exp(-(1.0 / 24.0) / 0.5))) and Display(adaptation=0.5).adapt(-1.0 / 24.0) == a
    p = Display(exposure="auto", key=0.25, tone="reinhard", bloom=Bloom(2.0, 0.25, 3)).to_abi(0.5)
    assert (p.tone, p.auto_exposure, p.key, p.adapt, p.levels, p.threshold, p.strength) == (1, 1, 0.25, 0.5, 3, 2.0, 0.25)
    for bad in (dict(exposure="manual"), dict(exposure=float("nan")), dict(exposure=True), dict(exposure=1000), dict(key=0.0), dict(key=float("inf")),
                dict(key="1"), dict(tone="filmic"), dict(tone=2), dict(white=0.0), dict(white=float("nan")), dict(bloom=5), dict(adaptation=0.0),
                dict(adaptation=float("inf")), dict(adaptation="1")):
        with pytest.raises(ValueError, match="Display"):
            Display(**bad)
    for bad in (dict(levels=0), dict(levels=9), dict(levels=2.0), dict(levels=True), dict(threshold=-1.0), dict(threshold=float("nan")),
                dict(strength=-0.5), dict(strength=float("inf")), dict(strength="1")):
        with pytest.raises(ValueError, match="Bloom"):
            Bloom(**bad)


def test_abi_struct_matches_the_header_and_the_library():
    hdr = open(os.path.join(ROOT, "include", "rayn_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\}\s*rayn_display_params;", hdr).group(1)
    fields = [tuple(decl.split()) for decl in body.split(";") if decl.strip()]
    ctype = {"uint32_t": C.c_uint32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(_abi.DisplayParams._fields_)
    assert C.sizeof(_abi.DisplayParams) == 36
    _lib.build()
    assert _lib.lib().rayn_hip_sizeof(8) == 36
    for i, (name, _) in enumerate(_abi.DisplayParams._fields_):
        assert getattr(_abi.DisplayParams, name).offset == 4 * i


def test_pfm_round_trip(tmp_path):
    rng = np.random.default_rng(5)
    rgb = np.exp(rng.uniform(-8, 8, (7, 5, 3))).astype(np.float32)
    rgb[0, 0] = (np.nan, np.inf, -0.0)
    path = tmp_path / "x.pfm"
    image.save_pfm(path, rgb)
    raw = open(path, "rb").read()
    assert raw.startswith(b"PF\n5 7\n-1.0\n") and len(raw) == len(b"PF\n5 7\n-1.0\n") + 7 * 5 * 12
    assert raw[len(b"PF\n5 7\n-1.0\n"):] == rgb.astype("<f4").tobytes()  # the film's own row order: bottom-up, as PFM has it
    assert np.array_equal(image.load_pfm(path).view(np.uint32), rgb.view(np.uint32))
    with pytest.raises(ValueError):
        image.save_pfm(path, rgb[..., 0])
