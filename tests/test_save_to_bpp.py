"""rayn_save_to_bpp (include/rayn_hip.h), the host-only half of the device save_to post-process: for every (ChannelKind, channel set,
transparent_background) it returns the bytes per pixel oracle_save_to_pixels writes, and -1 exactly where the oracle (the reference's
Film::save_to, src/film.rs:205-378) returns Err."""
import ctypes as C

import numpy as np

from rayn_amd import film as F


def _oracle_bpp(oracle, kind, mask, transparent):
    L = oracle.lib()
    L.oracle_save_to_pixels.restype = C.c_int
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    w, h = 2, 3
    color, alpha, background, normal = (np.full(w * h * c, 0.25, np.float32) for c in (3, 1, 3, 3))
    out = np.zeros(w * h * 4, np.uint8)
    return L.oracle_save_to_pixels(C.c_uint32(kind), mask & 1, (mask >> 1) & 1, (mask >> 2) & 1, (mask >> 3) & 1, int(transparent), C.c_uint32(w), C.c_uint32(h),
                                   fp(color), fp(alpha), fp(background), fp(normal), out.ctypes.data_as(C.POINTER(C.c_uint8)))


def test_bpp_matches_the_oracle_for_every_combination(oracle):
    seen = set()
    for kind in range(4):
        for mask in range(16):
            for transparent in (False, True):
                want = _oracle_bpp(oracle, kind, mask, transparent)
                assert F.save_to_bpp(kind, mask, transparent) == want, (kind, mask, transparent, want)
                assert F.save_to_bpp(F.ChannelKind(kind), mask, transparent) == want
                seen.add(want)
    assert seen == {-1, 1, 3, 4}


def test_film_save_jobs_follow_the_reference_arms():
    """Film._save_jobs needs no GPU context: check the arm selection through a Film-like object built without one."""
    K = F.ChannelKind
    film = F.Film.__new__(F.Film)
    film.channel_kinds = [K.Color]
    assert film.have_mask() == 1
    assert film._save_jobs([K.Color], False) == [(K.Color, 3, "color")]
    for kinds, transparent, text in (([K.Color], True, "Attempted to write Color channel with insufficient channels"),
                                     ([K.Alpha], False, "Attempted to write Alpha channel but it didn't exist"),
                                     ([K.Background], False, "Attempted to write Background channel but it didn't exist"),
                                     ([K.WorldNormal], False, "Attempted to write WorldNormal channel but it didn't exist")):
        try:
            film._save_jobs(kinds, transparent)
        except ValueError as e:
            assert str(e) == text
        else:
            raise AssertionError(kinds)
    film.channel_kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    assert film._save_jobs([K.Color, K.Alpha], True) == [(K.Color, 4, "color"), (K.Alpha, 1, "alpha")]
    assert [b for _, b, _ in film._save_jobs(list(K), False)] == [3, 1, 3, 3]
