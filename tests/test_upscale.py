"""The guided upscaling's definition (include/rayn_hip.h) through its numpy restatement tests/upscale_np.py, on the CPU: the factor-1
identity, partition of unity, a step edge between two objects that plain bilinear smears and the guided weights keep, the three tiers,
the image borders, the plane term, the validation of rayn_amd.Upscale, the float64 reading, and what the high G-buffer is - the
oracle's G-buffer at s times the resolution through the low film's world description has the rays of a world built at the high
resolution but the low film's hit threshold.  tests/test_upscale_device.py compares the kernel with the same restatement bit for bit."""
import numpy as np
import pytest

import scenes
import temporal_np as T
import upscale_np as U

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _plane_gbuffers(w, h, s, obj=1, pixel=0.125):
    """The G-buffers of the orthographic camera over the plane z = 0 at w x h and at s times that (the same world extent)."""
    lrec, lobj, lnrm = T.ortho_plane_gbuffer(w, h, pixel=pixel, obj=obj)
    hrec, hobj, _ = T.ortho_plane_gbuffer(w * s, h * s, pixel=pixel / s, obj=obj)
    return (lrec, lobj), (hrec, hobj), lnrm


def _random_film(rng, n, normal):
    return {"color": rng.gamma(0.6, 0.5, (n, 3)).astype(f32), "alpha": rng.random(n).astype(f32),
            "background": rng.random((n, 3)).astype(f32), "normal": (normal + rng.normal(0.0, 0.3, (n, 3))).astype(f32)}


def test_factor_one_is_the_identity_in_every_bit():
    """Random films with -0.0, denormal, NaN and inf colours, random objects, misses and depth noise: every plane of every pixel comes
    out with the bits it went in with - a finite colour through tier 1 (b_0 = 1, expf(-0) = 1, sums that start at -0.0f), a non-finite
    one verbatim through tier 3 - with each sigma on and off."""
    for seed, (w, h) in enumerate([(24, 16), (25, 19), (1, 1)]):
        rng = np.random.default_rng(seed)
        n = w * h
        (rec, obj), _, nrm = _plane_gbuffers(w, h, 1)
        rec[:, 2] = rng.normal(0.0, 0.05, n)
        obj = rng.choice(np.array([0, 1, 1, 2, 0xFFFFFFFF], np.uint32), n)
        rec[obj == U.MISS] = (0.0, 0.0, 0.0, np.inf)
        film = _random_film(rng, n, nrm)
        special = np.array([np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-45, -1e-40, 3.0e38], f32)
        flat = film["color"].reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 40), replace=False)
        flat[idx] = np.resize(special, idx.size)
        film["alpha"][rng.choice(n, min(n, 5), replace=False)] = -0.0
        for sp, ss in ((0.0, 0.0), (0.02, 0.0), (0.0, 0.05), (0.02, 0.05)):
            out, weight, tier, _ = U.upscale(film, (rec, obj), (rec, obj), w, h, 1, sp, ss)
            for k in film:
                assert np.array_equal(_bits(out[k]), _bits(film[k])), (w, h, sp, ss, k)
            fin = np.isfinite(film["color"]).all(axis=1)
            assert np.all(tier[fin] == 1) and np.all(tier[~fin] == 3) and np.all(weight[fin] == 1.0) and np.all(weight[~fin] == 0.0)
        assert n == 1 or (not fin.all() and fin.any())


@pytest.mark.parametrize("s", [2, 3, 4])
def test_partition_of_unity(s):
    """A film whose every plane is 1.0 on one flat object comes out exactly 1.0: the weights of a pixel are normalised by their own sum."""
    w, h = 25, 19
    low, high, nrm = _plane_gbuffers(w, h, s)
    film = {"color": np.ones((w * h, 3), f32), "alpha": np.ones(w * h, f32), "background": np.ones((w * h, 3), f32), "normal": np.ones((w * h, 3), f32)}
    for sp, ss in ((0.0, 0.0), (0.05, 0.1)):
        out, weight, tier, _ = U.upscale(film, low, high, w, h, s, sp, ss)
        assert all(np.all(out[k] == 1.0) for k in film) and np.all(tier == 1) and np.all(weight > 0)


@pytest.mark.parametrize("s", [2, 3, 4])
def test_step_edge_between_two_objects_stays_sharp(s):
    """The plane split into objects A (Color 1) and B (Color 0) at the high column E, which falls inside a low pixel: every high pixel
    comes out exactly 1.0 or 0.0 according to its own object, where the plain bilinear reading of the same film gives values in between."""
    w, h = 24, 16
    W = w * s
    E = s * 11 + 1
    (lrec, _), (hrec, _), nrm = _plane_gbuffers(w, h, s)
    lobj = np.where((np.arange(w) + 0.5) * s < E, 1, 2).astype(np.uint32)  # the object under the low pixel's centre
    lobj = np.tile(lobj, h)
    hobj = np.tile(np.where(np.arange(W) < E, 1, 2).astype(np.uint32), h * s)
    film = {"color": np.repeat((lobj == 1).astype(f32)[:, None], 3, axis=1), "normal": nrm}
    out, weight, tier, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.0)
    want = np.repeat((hobj == 1).astype(f32)[:, None], 3, axis=1)
    assert np.array_equal(out["color"], want) and np.all(tier == 1)
    plain, _, ptier, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.0, bilinear=True)
    mixed = (plain["color"][:, 0] > 0) & (plain["color"][:, 0] < 1)
    assert mixed.sum() >= h * s and np.all(ptier == 2)  # at least one smeared pixel per high row: the test bites


def test_the_fallback_tiers():
    """A high pixel whose object no tap shares takes the plain bilinear weights (tier 2) and reports a weight of 0; a pixel whose four
    taps all hold a non-finite colour is the low pixel it falls into, verbatim (tier 3)."""
    w, h, s = 24, 16, 2
    W = w * s
    rng = np.random.default_rng(5)
    (lrec, lobj), (hrec, hobj), nrm = _plane_gbuffers(w, h, s)
    film = _random_film(rng, w * h, nrm)
    lone = 7 + 9 * W  # an interior high pixel showing an object no low pixel shows
    hobj[lone] = 9
    for x in (4, 5, 6):
        for y in (10, 11, 12):
            film["color"][x + y * w] = (np.nan, 1.0, np.inf)
    dead = (2 * 5 + 1) + (2 * 11) * W  # its four taps are low pixels (5..6, 10..11)
    out, weight, tier, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.1)
    plain, _, _, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.1, bilinear=True)
    assert tier[lone] == 2 and weight[lone] == 0.0 and all(np.array_equal(_bits(out[k][lone]), _bits(plain[k][lone])) for k in film)
    assert tier[dead] == 3 and weight[dead] == 0.0
    for k in film:
        assert np.array_equal(_bits(out[k][dead]), _bits(film[k][5 + 11 * w])), k
    assert (tier == 1).sum() > W * h * s * 0.9 and np.all(weight[tier == 1] > 0)


def _scalar_bilinear(film_plane, w, h, s, X, Y):
    """One pixel of one plane by the definition's steps 1 and 3 with g_k = b_k, in scalar float32: an independent reading for the borders."""
    fx, fy = f32(f32(f32(X) + f32(0.5)) / f32(s)) - f32(0.5), f32(f32(f32(Y) + f32(0.5)) / f32(s)) - f32(0.5)
    x0, y0 = int(np.floor(fx)), int(np.floor(fy))
    wx1, wy1 = f32(fx - f32(x0)), f32(fy - f32(y0))
    wx = (f32(f32(1.0) - wx1), wx1)
    wy = (f32(f32(1.0) - wy1), wy1)
    Wt, St, used = f32(-0.0), f32(-0.0), []
    for k in range(4):
        qx, qy = x0 + (k & 1), y0 + (k >> 1)
        b = f32(wx[k & 1] * wy[k >> 1])
        if 0 <= qx < w and 0 <= qy < h and b > 0:
            Wt, St = f32(Wt + b), f32(St + f32(b * film_plane[qx + qy * w]))
            used.append(k)
    return f32(St / Wt), Wt, used


def test_taps_outside_the_image_are_skipped_at_all_four_borders():
    """Factor 3: the first and last high column and row look one low pixel past the image.  Those taps drop out - the pixel is the
    normalised blend of the taps inside - instead of being clamped or read as zero."""
    w, h, s = 20, 12, 3
    W, H = w * s, h * s
    rng = np.random.default_rng(11)
    low, high, nrm = _plane_gbuffers(w, h, s)
    film = {"color": rng.random((w * h, 3)).astype(f32) + f32(0.5), "alpha": rng.random(w * h).astype(f32)}
    out, weight, tier, _ = U.upscale(film, low, high, w, h, s, 0.0, 0.0)
    seen = set()
    for X, Y in [(0, 8), (W - 1, 8), (11, 0), (11, H - 1), (0, 0), (W - 1, H - 1), (0, H - 1), (W - 1, 0), (11, 8)]:
        want, Wt, used = _scalar_bilinear(film["alpha"], w, h, s, X, Y)
        assert _bits(out["alpha"][X + Y * W]) == _bits(want) and _bits(weight[X + Y * W]) == _bits(Wt), (X, Y)
        seen.add(len(used))
    assert seen == {1, 2, 4} and np.all(tier == 1)
    assert weight[0 + 8 * W] < 0.75 and abs(float(weight[11 + 8 * W]) - 1.0) < 1e-6  # two of four taps; all four


def test_the_plane_term_separates_parallel_planes_of_one_object():
    """One object, two parallel planes a unit of depth apart, Color 1 on the near and 0 on the far one, the depth step inside a low
    pixel: with a small sigma_plane the far taps' weights underflow to 0 and no pixel mixes the two; with the term off they mix."""
    w, h, s = 24, 16, 2
    W = w * s
    E = s * 11 + 1
    (lrec, lobj), (hrec, hobj), nrm = _plane_gbuffers(w, h, s)
    lfar = np.tile((np.arange(w) + 0.5) * s >= E, h)
    hfar = np.tile(np.arange(W) >= E, h * s)
    for rec, far in ((lrec, lfar), (hrec, hfar)):
        rec[far, 2], rec[far, 3] = -1.0, 5.0
    film = {"color": np.repeat((~lfar).astype(f32)[:, None], 3, axis=1), "normal": nrm}
    out, _, tier, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.01, 0.0)
    assert np.array_equal(out["color"][:, 0], (~hfar).astype(f32)) and np.all(tier == 1)
    off, _, _, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.0, 0.0)
    assert ((off["color"][:, 0] > 0) & (off["color"][:, 0] < 1)).sum() >= h * s


def test_upscale_parameter_validation():
    import rayn_amd as R
    assert R.Upscale().factor == 2
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match=r"Upscale.factor must be an int in 1..8"):
            R.Upscale(factor=bad)
    for name in ("sigma_plane", "sigma_position"):
        for bad in (-1.0, float("nan"), float("inf"), 2.0 ** -31, 2.0 ** 31):
            with pytest.raises(ValueError, match=rf"Upscale.{name} must be 0 \(off\) or finite in \[2\^-30, 2\^30\]"):
                R.Upscale(**{name: bad})
        with pytest.raises(ValueError, match=rf"Upscale.{name} must be a number"):
            R.Upscale(**{name: "1"})
        R.Upscale(**{name: 0.0})
    u = R.Upscale(3, 0.25, 0.5)
    assert u.without(0b1111) == u and u.without(0b0111) == R.Upscale(3, 0.0, 0.5)
    a = u.to_abi()
    assert (a.factor, a.sigma_plane, a.sigma_position) == (3, 0.25, 0.5)
    import inspect
    sig = inspect.signature(R.Film.render_sequence)
    assert sig.parameters["upscale"].default is None


def test_the_float64_reading_agrees():
    """The same formulas in float64.  The tolerance is derived, with u = 2^-24, for inputs in [0, 1] (sums of non-negative terms: no
    cancellation) whose exponents stay below E (no underflow, so both readings take the same tier):
      - fx carries the rounding of the division and of the subtraction, at most 2 u wmax in absolute terms (wmax the low width or
        height); fx - floor(fx) is exact, so a bilinear factor of at least 1 / (2 s) has a relative error of at most 4 s wmax u, and
        b_k, a product of two and one rounding, at most 8 s wmax u + u.  floor() itself cannot differ: an fx that is an integer is exact
        in both readings, any other lies 1 / (2 s) away from one.
      - e is a dozen operations on the guides, a relative error of at most 12 u, so expf(-e) is off by at most 12 E u, plus u for the
        correctly rounded dm_expf and u for the product with b_k: g_k has a relative error of at most (8 s wmax + 12 E + 3) u.
      - S / W: the errors of the g_k enter numerator and denominator (twice the above at worst), each of the four terms adds a product
        and a sum rounding in S and a sum rounding in W, and the division one more: 2 (8 s wmax + 12 E + 3) u + 13 u.
    With values of at most 1 that relative bound is the absolute one: (16 s wmax + 24 E + 19) u."""
    E = 8.0
    for seed, (w, h, s) in enumerate([(24, 16, 2), (25, 19, 3), (20, 12, 4)]):
        rng = np.random.default_rng(20 + seed)
        n = w * h
        (lrec, lobj), (hrec, hobj), nrm = _plane_gbuffers(w, h, s)
        lrec[:, 2], hrec[:, 2] = rng.normal(0.0, 0.02, n), rng.normal(0.0, 0.02, n * s * s)
        lobj = np.tile(np.where(np.arange(w) < w // 2, 1, 2).astype(np.uint32), h)
        hobj = np.tile(np.where(np.arange(w * s) < s * (w // 2) + 1, 1, 2).astype(np.uint32), h * s)
        film = {"color": rng.random((n, 3)).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
                "normal": np.clip(nrm * f32(0.8) + rng.normal(0.0, 0.1, (n, 3)), 0.0, 1.0).astype(f32)}
        a, wa, ta, emax = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.05)
        b, wb, tb, _ = U.upscale(film, (lrec, lobj), (hrec, hobj), w, h, s, 0.05, 0.05, dtype=np.float64)
        assert 0.5 < emax < E and np.array_equal(ta, tb) and set(np.unique(ta)) == {1}
        tol = (16 * s * max(w, h) + 24 * E + 19) * 2.0 ** -24
        for k in film:
            assert np.max(np.abs(a[k].astype(np.float64) - b[k])) <= tol, (w, h, s, k)
        assert np.max(np.abs(wa.astype(np.float64) - wb)) <= 4 * tol  # the weight itself: four terms, each within the bound on g_k


def _scene(name, res, camera="pinhole"):
    """The world description of a test scene at a resolution, with the camera variants of scenes.scene"""
    return scenes.scene(name, res, camera)[0]


@pytest.mark.parametrize("scene,camera,res,s", [("s1", "pinhole", (12, 8), 2), ("s2", "pinhole", (10, 6), 3), ("s1", "thin", (9, 7), 2),
                                                ("s1", "ortho", (12, 8), 4), ("s1", "thin", (10, 6), 3), ("s2", "ortho", (9, 7), 2)])
def test_the_high_gbuffer_through_the_low_films_world(oracle, scene, camera, res, s):
    """The upscaled film's guide is rayn_hip_gbuffer_device under the LOW film's uploaded world with the frame's width and height
    multiplied by s.  Is that the G-buffer of a world built at the high resolution?  Measured here, not assumed - and it is NOT:
      - the two world descriptions differ in the camera's resolution alone, and the factor keeps the aspect ratio, so half_w .. full_h
        are the same and the pixel-centre rays are the same, bit for bit;
      - but the camera's resolution also sets half_pixel_size, the hit threshold of a depth-0 march (src/film.rs:540-551), so the march
        under the low film's world stops where the LOW render's primary rays stop: never farther along a ray than under the high world,
        and on these scenes strictly nearer for a third of the pixels and more.
    The definition therefore says which one it takes - the low film's world (DESIGN.md section 8 says why: both G-buffers then describe
    the surface the film's samples were shaded on, so P - Pq measures geometry and not the difference of two thresholds) - and this test
    pins the three facts, so that a change of either is seen."""
    import rayn_amd as R
    w, h = res
    p_high = R.frame_params(w * s, h * s, 1, 2, frame=3)
    wd_low, wd_high = _scene(scene, (w, h), camera), _scene(scene, (w * s, h * s), camera)
    for a, b in zip(T.pixel_centre_rays(oracle, wd_low, p_high), T.pixel_centre_rays(oracle, wd_high, p_high)):
        assert np.array_equal(_bits(a), _bits(b))
    rec_a, obj_a = T.gbuffer_oracle(oracle, wd_low, p_high)
    rec_b, obj_b = T.gbuffer_oracle(oracle, wd_high, p_high)
    same = obj_a == obj_b
    # 0.98 and 0.3 are empirical floors, read off these six cases (at least 0.981 of the objects agree, at least 0.39 of the hits are
    # strictly nearer), not derived: they say "nearly every object" and "a large share", and the <= beside them is the exact part
    assert same.mean() > 0.98 and len(set(obj_a.tolist())) >= 2
    assert np.all(rec_a[same, 3] <= rec_b[same, 3]) and (rec_a[same, 3] < rec_b[same, 3]).mean() > 0.3
    # the resolution is the only difference: the low description with its camera's resolution multiplied by s IS the high one
    wd_low.camera.res_w *= s
    wd_low.camera.res_h *= s
    assert bytes(memoryview(wd_low).cast("B")) == bytes(memoryview(wd_high).cast("B"))
