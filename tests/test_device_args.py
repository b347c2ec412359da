"""The checks every device entry's tensor arguments go through (rayn_amd.context), on CPU tensors: none touches a Context or the GPU.
The ValueError texts are the wrappers', as full strings."""
import pytest
import torch

from rayn_amd import context as X
from rayn_amd import film as F

N_PIX = 6  # a 3 x 2 film


def _raises(text, fn, *args):
    with pytest.raises(ValueError) as e:
        fn(*args)
    assert str(e.value) == text


def _bad(count, dtype=torch.float32):
    """The three tensors a check of `count` elements refuses: a wrong dtype, a non-contiguous view, one element short."""
    other = torch.float64 if dtype != torch.float64 else torch.float32
    return [torch.zeros(count, dtype=other), torch.zeros(2 * count, dtype=dtype)[::2], torch.zeros(count - 1, dtype=dtype)]


def test_film_re_exports_the_helpers():
    for name in ("f32_ptr", "opt_f32_ptr", "i32_ptr", "film_ptrs", "gbuffer_ptrs", "byte_ptrs", "scratch", "stream_ptr", "Context", "RdTablePrefetch"):
        assert getattr(F, name) is getattr(X, name)


def test_f32_ptr():
    t = torch.zeros(N_PIX, 3)
    assert X.f32_ptr(t, "d_out_color", 18).value == t.data_ptr()
    big = torch.zeros(40)[4:]  # larger, and not at the start of its storage
    assert X.f32_ptr(big, "d_out_color", 18).value == big.data_ptr()
    for t in _bad(18) + [None]:
        _raises("d_out_color must be a contiguous float32 tensor of at least 18 floats", X.f32_ptr, t, "d_out_color", 18)
    assert X.opt_f32_ptr(None, "d_out_weight", 24) is None
    w = torch.zeros(24)
    assert X.opt_f32_ptr(w, "d_out_weight", 24).value == w.data_ptr()
    for t in _bad(24):
        _raises("d_out_weight must be a contiguous float32 tensor of at least 24 floats", X.opt_f32_ptr, t, "d_out_weight", 24)
    for t in _bad(2):
        _raises("d_out_meter must be a contiguous float32 tensor of at least 2 floats", X.opt_f32_ptr, t, "d_out_meter", 2)
    # temporal_accumulate names its planes without the dict
    _raises("'color' must be a contiguous float32 tensor of at least 18 floats", X.f32_ptr, None, "'color'", 18)


def test_film_ptrs():
    film = {"color": torch.zeros(N_PIX, 3), "alpha": torch.zeros(N_PIX), "background": torch.zeros(N_PIX, 3), "normal": torch.zeros(N_PIX, 3)}
    got = X.film_ptrs(film, X.FILM_KEYS, N_PIX, "d_film")
    assert [p.value for p in got] == [film[k].data_ptr() for k in ("color", "alpha", "background", "normal")]
    got = X.film_ptrs(film, X.GUIDE_KEYS, N_PIX, "d_film")
    assert [p.value for p in got] == [film[k].data_ptr() for k in ("color", "alpha", "normal")]
    got = X.film_ptrs({"color": film["color"], "normal": film["normal"]}, X.FILM_KEYS, N_PIX, "d_out_film")
    assert [None if p is None else p.value for p in got] == [film["color"].data_ptr(), None, None, film["normal"].data_ptr()]
    assert X.film_ptrs({}, X.FILM_KEYS, N_PIX, "d_film") == [None] * 4
    for key, floats in (("color", 18), ("alpha", 6), ("background", 18), ("normal", 18)):
        for t in _bad(floats):
            for label in ("d_film", "d_out_film"):
                _raises(f"{label}['{key}'] must be a contiguous float32 tensor of at least {floats} floats", X.film_ptrs, dict(film, **{key: t}),
                        X.FILM_KEYS, N_PIX, label)
    # the first bad plane in key order is the one named
    _raises("d_film['alpha'] must be a contiguous float32 tensor of at least 6 floats", X.film_ptrs,
            dict(film, alpha=torch.zeros(5), normal=torch.zeros(1)), X.FILM_KEYS, N_PIX, "d_film")


def test_gbuffer_ptrs():
    g = {"records": torch.zeros(N_PIX, 4), "object": torch.zeros(N_PIX, dtype=torch.int32)}
    rec, obj = X.gbuffer_ptrs(g, N_PIX, "d_gbuffer")
    assert (rec.value, obj.value) == (g["records"].data_ptr(), g["object"].data_ptr())
    for t in _bad(24) + [None]:
        _raises("d_low_gbuffer['records'] must be a contiguous float32 tensor of at least 24 floats", X.gbuffer_ptrs, dict(g, records=t), N_PIX,
                "d_low_gbuffer")
    for t in _bad(6, torch.int32) + [None]:
        _raises("d_high_gbuffer['object'] must be a contiguous int32 tensor of at least 6 elements", X.gbuffer_ptrs, dict(g, object=t), N_PIX,
                "d_high_gbuffer")
    _raises("d_gbuffer['records'] must be a contiguous float32 tensor of at least 24 floats", X.gbuffer_ptrs, {}, N_PIX, "d_gbuffer")
    assert X.i32_ptr(g["object"], "d_gbuffer['object']", N_PIX).value == g["object"].data_ptr()


def test_byte_ptrs_take_the_smaller_of_new_and_prev():
    new, prev, short = torch.zeros(96, dtype=torch.uint8), torch.zeros(96, dtype=torch.uint8), torch.zeros(64, dtype=torch.uint8)
    p, n, nbytes = X.byte_ptrs(new, "d_new_history")
    assert (p, n.value, nbytes) == (None, new.data_ptr(), 96)
    p, n, nbytes = X.byte_ptrs(new, "d_new_history", prev, "d_prev_history")
    assert (p.value, n.value, nbytes) == (prev.data_ptr(), new.data_ptr(), 96)
    assert X.byte_ptrs(new, "d_new_history", short, "d_prev_history")[2] == 64
    assert X.byte_ptrs(short, "d_new_moments", prev, "d_prev_moments")[2] == 64
    for label in ("d_new_history", "d_new_moments", "d_history", "d_moments", "d_state"):
        for t in (None, torch.zeros(96, dtype=torch.int8), torch.zeros(192, dtype=torch.uint8)[::2]):
            _raises(f"{label} must be a contiguous uint8 tensor", X.byte_ptrs, t, label)
    for t in (torch.zeros(96, dtype=torch.float32), torch.zeros(192, dtype=torch.uint8)[::2]):
        _raises("d_prev_history must be a contiguous uint8 tensor", X.byte_ptrs, new, "d_new_history", t, "d_prev_history")
    _raises("d_new_moments must be a contiguous uint8 tensor", X.byte_ptrs, None, "d_new_moments", prev, "d_prev_moments")
    # a bad prev is named before a bad new
    _raises("d_prev_history must be a contiguous uint8 tensor", X.byte_ptrs, None, "d_new_history", torch.zeros(4), "d_prev_history")


@pytest.mark.parametrize("nbytes", [0, 1, 1000])
def test_scratch_allocates_at_least_one_byte_on_the_device(nbytes):
    t, p, n = X.scratch(None, nbytes, torch.device("cpu"))
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.device == torch.device("cpu")
    assert t.numel() == n == max(nbytes, 1) and p.value == t.data_ptr()


def test_scratch_takes_what_it_is_given():
    mine = torch.zeros(10, dtype=torch.float32)  # any contiguous tensor: its size in bytes counts
    t, p, n = X.scratch(mine, 1000, torch.device("cpu"))
    assert t is mine and p.value == mine.data_ptr() and n == 40
    _raises("d_scratch must be contiguous", X.scratch, torch.zeros(20, dtype=torch.uint8)[::2], 4, torch.device("cpu"))


def test_stream_ptr_passes_a_given_stream_through():
    assert X.stream_ptr(0).value is None and X.stream_ptr(0x1234).value == 0x1234


def test_wrappers_raise_the_helpers_texts_without_a_context():
    """The checks run before the entry is called: a Context made without a GPU reaches them."""
    ctx = X.Context.__new__(X.Context)
    ctx.h = None
    film = {"color": torch.zeros(N_PIX, 3), "alpha": torch.zeros(N_PIX - 1)}
    out = torch.zeros(N_PIX, 3)
    _raises("d_film['alpha'] must be a contiguous float32 tensor of at least 6 floats", ctx.denoise, 3, 2, film, out, F.Denoise())
    _raises("d_out_color must be a contiguous float32 tensor of at least 18 floats", ctx.denoise, 3, 2, film, out[:5], F.Denoise())
    p = F.frame_params(3, 2, 1, 2)
    g = {"records": torch.zeros(N_PIX, 4), "object": torch.zeros(N_PIX, dtype=torch.int32)}
    _raises("'normal' must be a contiguous float32 tensor of at least 18 floats", ctx.temporal_accumulate, p, F.Temporal(), film, g, None, None, 0.0,
            torch.zeros(8, dtype=torch.uint8), out)
    full = dict(film, normal=torch.zeros(N_PIX, 3))
    _raises("d_new_history must be a contiguous uint8 tensor", ctx.temporal_accumulate, p, F.Temporal(), full, g, None, None, 0.0, None, out)
    _raises("d_out_film['color'] must be a contiguous float32 tensor of at least 72 floats", ctx.upscale, p, F.Upscale(2), {"color": out}, g, g,
            {"color": out})
    _raises("d_high_gbuffer['records'] must be a contiguous float32 tensor of at least 96 floats", ctx.upscale, p, F.Upscale(2), {"color": out}, g, g,
            {"color": torch.zeros(4 * N_PIX, 3)})
