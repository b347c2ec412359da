"""The temporal supersampling's definition (include/rayn_hip.h) through its numpy restatement tests/temporal_upscale_np.py, on the CPU: with
no low camera and confidence off it is the upscale followed by the accumulate at the high size, bit for bit; the projected footprint
against the default one; confidence at factor 1; the geometry of the jittered camera through the oracle's rays; and the validation of
rayn_amd.Supersample and of render_sequence's argument combinations.  tests/test_temporal_upscale_device.py compares the kernel with the
same restatement bit for bit."""
import numpy as np
import pytest

import temporal_np as T
import temporal_upscale_np as TU
import upscale_np as U
from common import bits_equal, case
from temporal_upscale_cases import FACTORS, SIGMAS, SIZES, sequence

f32 = np.float32
NOHIT = []


def same_history(a, b):
    return all(bits_equal(x.astype(f32) if x.dtype != np.uint32 else x.view(f32), y.astype(f32) if y.dtype != np.uint32 else y.view(f32)) for x, y in zip(a, b))


def test_without_low_camera_and_confidence_it_is_upscale_then_accumulate():
    """Every low size x every factor, random and adversarial, the sigma pairs in turn, films with and without Alpha / Background, three
    chained frames under a moving camera with a history capped at 2: every output plane, the weight and the whole new history have the
    bits of U.upscale followed by T.accumulate at the high size.  Over the cases tiers 1, 2 and 3, a reset of a hit pixel that had a
    history to look at, a capped history and a rejected history tap all occur."""
    seen = {"tiers": set(), "reset": False, "capped": False, "rejected": False}
    ci = 0
    for si, (w, h) in enumerate(SIZES):
        for s in FACTORS:
            for adversarial in (False, True):
                sp, ss = SIGMAS[ci % 4]
                lack = [(), ("alpha", "background"), ("background",)][ci % 3]
                mh, tol, nmin = [(2, 0.05, -1.0), (2, 0.01, 0.5), (32, 0.05, 0.9)][ci % 3]
                ci += 1
                prev_a = prev_b = None
                prev_cam, prev_time = None, 0.0
                for film, low_g, high_g, cam, ts in sequence(w, h, s, 100 * si + 10 * s + adversarial, adversarial):
                    part = {k: v for k, v in film.items() if k not in lack}
                    W, H = w * s, h * s
                    planes, weight, hist, info = TU.temporal_upscale(part, low_g, high_g, w, h, s, sp, ss, None, ts, False, prev_a, prev_cam, prev_time,
                                                                     NOHIT, mh, tol, nmin)
                    up, up_weight, tier, _ = U.upscale(part, low_g, high_g, w, h, s, sp, ss)
                    out, hist_b = T.accumulate(W, H, up["color"], up["normal"], high_g[0], high_g[1], prev_b, prev_cam, prev_time, ts, NOHIT, mh, tol, nmin)
                    what = (w, h, s, adversarial, sp, ss, lack, ts)
                    assert bits_equal(planes["color"], out), what
                    for k in part:
                        if k != "color":
                            assert bits_equal(planes[k], up[k]), (what, k)
                    assert bits_equal(weight, up_weight) and np.array_equal(info["tier"], tier), what
                    assert same_history(hist, hist_b), what
                    assert np.all(info["conf"] == 1.0)
                    seen["tiers"] |= set(np.unique(tier).tolist())
                    if prev_a is not None:
                        hit = (high_g[1] != U.MISS) & np.isfinite(info["frame_color"]).all(axis=1)
                        seen["reset"] |= bool((hit & (info["n"] == 1.0)).any())
                        seen["capped"] |= bool(((info["n"] == f32(mh)) & (info["taps"] > 0)).any()) and mh == 2 and ts > 0.25
                        seen["rejected"] |= bool(info["rejected"].any())
                    prev_a, prev_b, prev_cam, prev_time = hist, hist_b, cam, ts
    assert seen == {"tiers": {1, 2, 3}, "reset": True, "capped": True, "rejected": True}, seen


def test_projected_footprint_through_the_same_camera_is_the_default_footprint():
    """A low camera equal to the camera of the high G-buffer, over the orthographic plane: the projection of a high pixel's hit point
    lands where the default footprint puts the pixel.  At 16 x 8 and factors 1, 2 and 4 every operation of both is exact and the two
    footprints are identical; over 24 x 16, 20 x 12 and 25 x 19 at factors 1 to 4 (and factor 3 at 16 x 8, whose division is not exact)
    they differ by at most 1.9e-6 low pixels (observed: one ulp of a coordinate between 16 and 32) - asserted below 1e-4, far under a
    pixel.  Every hit pixel is projected; a miss keeps the default."""
    for w, h in [(16, 8)] + SIZES:
        for s in FACTORS:
            W, H = w * s, h * s
            hrec, hobj, _ = T.ortho_plane_gbuffer(W, H, pixel=0.125 / s)
            hobj[::7] = U.MISS
            hrec[hobj == U.MISS] = (0.0, 0.0, 0.0, np.inf)
            cam = T.ortho_camera(w, h)
            dx, dy, _ = TU.footprint(w, h, s, (hrec, hobj), None, 0.0)
            px, py, projected = TU.footprint(w, h, s, (hrec, hobj), cam, 0.0)
            assert np.array_equal(projected, hobj != U.MISS)
            err = max(float(np.abs(px - dx).max()), float(np.abs(py - dy).max()))
            assert err < 1e-4, (w, h, s, err)
            if (w, h) == (16, 8) and s != 3:
                assert err == 0.0, (s, err)
            assert bits_equal(px[~projected], dx[~projected]) and bits_equal(py[~projected], dy[~projected])


def test_confidence_with_every_conf_one_is_confidence_off():
    """Factor 1: the default footprint hits every low pixel's centre, b_0 = 1, so conf = 1 in tiers 1 and 2 and by definition in tier 3,
    and confidence on gives the bits of confidence off - over two chained frames."""
    for seed, (w, h) in enumerate(SIZES):
        prev = [None, None]
        prev_cam, prev_time = None, 0.0
        for film, low_g, high_g, cam, ts in sequence(w, h, 1, 40 + seed, seed == 1, frames=2):
            res = [TU.temporal_upscale(film, low_g, high_g, w, h, 1, 0.02, 0.05, None, ts, conf, prev[conf], prev_cam, prev_time, NOHIT, 4, 0.05, -1.0)
                   for conf in (0, 1)]
            assert np.all(res[1][3]["conf"] == 1.0)
            assert all(bits_equal(res[0][0][k], res[1][0][k]) for k in res[0][0]) and same_history(res[0][2], res[1][2])
            prev, prev_cam, prev_time = [res[0][2], res[1][2]], cam, ts
        assert (res[0][3]["taps"] > 0).any()


def test_confidence_weighs_a_frame_by_its_nearest_low_sample():
    """Factor 2 on a constant history: conf is 9/16 everywhere inside (the default footprint's largest bilinear weight), the history
    length grows by it, and the blend weight is conf / n'."""
    w, h, s = 16, 8, 2
    W, H = w * s, h * s
    (lrec, lobj, nrm), (hrec, hobj, _) = T.ortho_plane_gbuffer(w, h), T.ortho_plane_gbuffer(W, H, pixel=0.0625)
    cam = T.ortho_camera(W, H, pixel=0.0625)
    film0 = {"color": np.zeros((w * h, 3), f32), "normal": nrm}
    film1 = {"color": np.ones((w * h, 3), f32), "normal": nrm}
    _, _, hist, _ = TU.temporal_upscale(film0, (lrec, lobj), (hrec, hobj), w, h, s, 0.0, 0.0, None, 0.0, True, None, None, 0.0, NOHIT, 8, 0.05, -1.0)
    planes, _, hist1, info = TU.temporal_upscale(film1, (lrec, lobj), (hrec, hobj), w, h, s, 0.0, 0.0, None, 0.0, True, hist, cam, 0.0, NOHIT, 8, 0.05, -1.0)
    inner = ((np.arange(W * H) % W > 0) & (np.arange(W * H) % W < W - 1) & (np.arange(W * H) // W > 0) & (np.arange(W * H) // W < H - 1))
    assert np.all(info["conf"][inner] == f32(0.5625)) and np.all(info["n"][inner] == f32(1.5625))
    assert np.all(planes["color"][inner] == f32(f32(0.5625) / f32(1.5625)))


def _ortho_world(res):
    import rayn_amd as R
    from rayn_amd import setup as S
    from rayn_amd.scene import OrthographicCamera
    cam, world = S.SCENES["s1"](res)
    c = world.cameras.get(cam)
    world.cameras[cam] = OrthographicCamera((float(res[0]), float(res[1])), 3.5, c.origin, c.at, c.up)
    return world.to_desc(cam)


def _plane_hits(org, dirs, point, normal):
    org, dirs = org.astype(np.float64), dirs.astype(np.float64)
    t = ((point - org) @ normal) / (dirs @ normal)
    return (org + t[:, None] * dirs).astype(f32)


@pytest.mark.parametrize("s", [2, 3])
def test_the_jittered_cameras_centre_rays_hit_the_high_pixel_centres(oracle, s):
    """Orthographic camera over a tilted plane, exact for every pixel: the centre rays of the low camera offset by phase (ix, iy) of
    Supersample.offsets meet the plane where the unjittered camera at the HIGH size sees the centres of the high pixels (s x + ix,
    s y + iy), within 1e-3 high pixels (f32 rounding at these magnitudes with a wide margin).  A pinhole camera: the same for the four
    pixels around the image centre.  The small rotation that stands in for the shift is exact AT the centre; half a low pixel beside it
    the perspective's second-order term is left (x * theta * (x + theta) in image-plane units: it falls with the square of the
    resolution, 1.2e-3 high pixels at 48 x 32 and factor 3, a quarter of that at 96 x 64), and - for a camera whose view direction is not perpendicular to `up` - a roll of
    (rotation angle) x tan(elevation), because the basis is rebuilt from the same `up`: scene s1's own camera, 5.6 degrees above the
    horizon, is 1.2e-3 high pixels off at 96 x 64 and factor 3 from that roll alone.  The pinhole case held to 1e-3 therefore looks along
    -z with up = +y at 96 x 64, where the roll vanishes and the second-order term is 3e-4, so that the bound tests the convention and not
    the tilt; the kernel projects through whatever camera it is given and depends on neither.  The two terms are pinned as well, so that
    a change of jittered_camera for tilted or small cameras is seen: the same untilted camera at 48 x 32 and s1's own tilted camera at
    96 x 64 must stay below 2e-3 high pixels.  Derived, for factor 3 and a jitter of a third of a low pixel: second order x theta (x +
    theta) with x = half a low pixel gives 1.2e-3 at 48 x 32 and 0.3e-3 at 96 x 64; the roll theta tan(elevation) = 5.9e-4 rad turns the
    1.5 high pixels to a neighbour's centre by 0.9e-3, 1.2e-3 with the second-order term (both observed to that figure).  2e-3 leaves the
    cross terms and f32 rounding room and is a fiftieth of what a wrong sign or axis of the shift would show."""
    import rayn_amd as R
    from rayn_amd import film as F
    offsets = R.Supersample.offsets(s)
    cells = [(round((jx + 0.5) * s - 0.5), round((jy + 0.5) * s - 0.5)) for jx, jy in offsets]
    assert sorted(cells) == [(ix, iy) for ix in range(s) for iy in range(s)]  # a permutation of the s^2 cells
    for kind, (w, h), bound in (("ortho", (12, 8), 1e-3), ("pinhole", (96, 64), 1e-3), ("pinhole", (48, 32), 2e-3), ("tilted pinhole", (96, 64), 2e-3)):
        wd = _ortho_world((w, h)) if kind == "ortho" else case("s1", w, h, 1, 1)[0]
        if kind == "pinhole":
            wd.camera.origin.x, wd.camera.origin.y, wd.camera.origin.z = 0.0, 0.0, 4.5
        p = R.frame_params(w, h, 1, 1, frame=2)
        cam = wd.camera
        o, at = np.array([cam.origin.x, cam.origin.y, cam.origin.z]), np.array([cam.at.x, cam.at.y, cam.at.z])
        view = (at - o) / np.linalg.norm(at - o)
        normal = view + (np.array([0.2, -0.1, 0.15]) if kind == "ortho" else 0.0)
        xs, ys = np.arange(w * h) % w, np.arange(w * h) // w
        near = (np.abs(xs - (w - 1) / 2) < 1) & (np.abs(ys - (h - 1) / 2) < 1) if kind != "ortho" else np.ones(w * h, bool)
        assert near.sum() == (4 if kind != "ortho" else w * h)
        for (jx, jy), (ix, iy) in zip(offsets, cells):
            low = type(wd).from_buffer_copy(wd)
            low.camera = F.jittered_camera(cam, jx, jy, p.time_start)
            org, dirs = T.pixel_centre_rays(oracle, low, p)
            P = _plane_hits(org, dirs, at, normal)
            ok, fx, fy, _ = T.project(cam, p.time_start, [P[:, 0], P[:, 1], P[:, 2]], w * s, h * s)
            assert ok.all()
            err = max(float(np.abs(fx - (xs * s + ix))[near].max()), float(np.abs(fy - (ys * s + iy))[near].max()))
            assert err < bound, (kind, (w, h), s, ix, iy, err)


def test_offsets_and_their_order():
    import rayn_amd as R
    assert R.Supersample.offsets(1) == [(0.0, 0.0)]
    assert R.Supersample.offsets(2) == [(-0.25, -0.25), (0.25, 0.25), (-0.25, 0.25), (0.25, -0.25)]
    for s in range(1, 9):
        off = R.Supersample.offsets(s)
        cells = [(round((jx + 0.5) * s - 0.5), round((jy + 0.5) * s - 0.5)) for jx, jy in off]
        assert len(set(cells)) == s * s and all(0 <= a < s and 0 <= b < s for a, b in cells)
        assert all(abs(jx - ((ix + 0.5) / s - 0.5)) < 1e-15 and abs(jy - ((iy + 0.5) / s - 0.5)) < 1e-15 for (jx, jy), (ix, iy) in zip(off, cells))
        if s >= 3:  # consecutive phases, the wrap included, share neither a row nor a column
            assert all(a[0] != b[0] and a[1] != b[1] for a, b in zip(cells, cells[1:] + cells[:1]))
    sup = R.Supersample()
    assert [sup.offset(2, i) for i in (0, 1, 4, 7)] == [R.Supersample.offsets(2)[i % 4] for i in (0, 1, 4, 7)]
    assert R.Supersample(jitter=False).offset(3, 5) == (0.0, 0.0)
    for bad in (0, 9, 2.0, True, None):
        with pytest.raises(ValueError, match="factor must be an int in 1..8"):
            R.Supersample.offsets(bad)


def test_supersample_validation():
    import dataclasses
    import rayn_amd as R
    sup = R.Supersample()
    assert isinstance(sup.jitter, bool) and isinstance(sup.confidence, bool)
    assert R.Supersample(confidence=True).to_abi().confidence == 1 and R.Supersample(confidence=False).to_abi().confidence == 0
    for name in ("jitter", "confidence"):
        for bad in (1, 0, None, "yes", 1.0):
            with pytest.raises(ValueError, match=rf"Supersample.{name} must be a bool"):
                R.Supersample(**{name: bad})
    with pytest.raises(dataclasses.FrozenInstanceError):
        sup.jitter = False
    from rayn_amd import _abi
    import ctypes as C
    assert C.sizeof(_abi.TemporalUpscaleParams) == 4


def test_render_sequence_rejects_bad_combinations_before_anything_runs(tmp_path):
    """The argument combinations raise before a context is touched: the film here has none."""
    import inspect
    import rayn_amd as R
    K = R.ChannelKind
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    assert inspect.signature(R.Film.render_sequence).parameters["supersample"].default is None
    film = R.Film.__new__(R.Film)
    film._init_state(kinds, (24, 16), None, "cuda:0")
    out = str(tmp_path / "no")

    def run(**kw):
        film.render_sequence(None, None, R.PathTracingIntegrator(max_bounces=2, volume_marches=2), None, (16, 16), [1, 2], 24, 1.0 / 24.0, 1, kinds, out,
                             "anim", **kw)

    sup, up, tmp = R.Supersample(), R.Upscale(2), R.Temporal()
    for kw, text in [(dict(supersample=sup), "pass both"), (dict(supersample=sup, upscale=up), "pass both"), (dict(supersample=sup, temporal=tmp), "pass both"),
                     (dict(supersample=True, upscale=up, temporal=tmp), "must be a Supersample"),
                     (dict(supersample=sup, upscale=up, temporal=4), "must be a Temporal"),
                     (dict(supersample=sup, upscale=2, temporal=tmp), "must be an Upscale"),
                     (dict(supersample=sup, upscale=up, temporal=tmp, denoise=R.VarianceDenoise()), "VarianceDenoise is not built"),
                     (dict(supersample=sup, upscale=up, temporal=R.Temporal(resample="catmull_rom")), "resample != 'bilinear' is not built"),
                     (dict(supersample=sup, upscale=up, temporal=R.Temporal(feedback=0.5)), "feedback > 0 is not built"),
                     (dict(upscale=up, temporal=tmp), "temporal= together with upscale= is not built: the temporal histories live at one resolution")]:
        with pytest.raises(ValueError, match=text):
            run(**kw)
    no_normal = R.Film.__new__(R.Film)
    no_normal._init_state([K.Color, K.Alpha], (24, 16), None, "cuda:0")
    with pytest.raises(ValueError, match="needs the film's Color and WorldNormal"):
        no_normal.render_sequence(None, None, R.PathTracingIntegrator(max_bounces=2, volume_marches=2), None, (16, 16), [1], 24, 1.0 / 24.0, 1, [K.Color],
                                  out, "anim", supersample=sup, upscale=up, temporal=tmp)
    import os
    assert not os.path.exists(out)
