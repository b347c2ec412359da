"""The frame generation on the CPU: the numpy restatement (tests/interpolate_np.py) against statements that share none of its code - the
exact orthographic case, whose every pixel can be written down - its special values, the Interpolate option, plan_sequence's rules and file
names, and which entries of a frame list are keys.  The kernel is compared with the restatement in tests/test_interpolate_device.py."""
import numpy as np
import pytest

import interpolate_np as I
import temporal_np as T

f32 = np.float32
W, H, PIXEL = 32, 16, 0.125
N = W * H


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def _case(seed=1):
    return I.ortho_case(W, H, seed, PIXEL)


def _img(a):
    a = np.asarray(a)
    return a.reshape(H, W, -1)


def _run(ka, kb, rec, obj, ts=0.5, tol=0.05, hitables=()):
    out, src = I.interpolate(W, H, ka, kb, rec, obj, ts, list(hitables), tol)
    return {k: _img(v) for k, v in out.items()}, src.reshape(H, W)


def test_every_pixel_of_the_exact_orthographic_case():
    """T halfway between key cameras 2 pixels apart: every interior pixel is exactly 0.5 * A[x + 1] + 0.5 * B[x - 1], in every plane; the
    column whose source leaves A's image takes B alone and the other way round."""
    ka, kb, rec, obj = _case()
    out, src = _run(ka, kb, rec, obj)
    assert np.all(src[:, 1:W - 1] == 0) and np.all(src[:, 0] == 1) and np.all(src[:, W - 1] == 2)
    for name in ("color", "alpha", "background", "normal"):
        A, B = _img(ka.film[name]), _img(kb.film[name])
        want = (f32(0.5) * A[:, 2:] + f32(0.5) * B[:, :W - 2]).astype(f32)
        assert np.array_equal(_bits(out[name][:, 1:W - 1]), _bits(want)), name
        assert np.array_equal(_bits(out[name][:, 0]), _bits(A[:, 1])), name  # B's source column -1 is outside: A alone
        assert np.array_equal(_bits(out[name][:, W - 1]), _bits(B[:, W - 2])), name
    # planes the film lacks are absent from the result
    ka.film = {"color": ka.film["color"]}
    kb.film = {"color": kb.film["color"]}
    only, src2 = _run(ka, kb, rec, obj)
    assert sorted(only) == ["color"] and np.array_equal(src2, src) and np.array_equal(_bits(only["color"]), _bits(out["color"]))


def test_occlusion_in_one_key_takes_the_other_and_in_both_cross_fades():
    """A second object covers the columns 10..13 of B only: the pixels whose B source lies there are A's alone (source 1).  Occluders over
    A's columns 21, 22 and B's columns 19, 20 hide T's columns 20, 21 in both keys: tier 2, the cross-fade of the keys' own pixels."""
    ka, kb, rec, obj = _case(2)
    o, r = kb.obj.reshape(H, W), kb.rec.reshape(H, W, 4)
    o[:, 10:14], r[:, 10:14, 3] = 2, 3.0
    o[:, 19:21], r[:, 19:21, 3] = 2, 3.0
    oa, ra = ka.obj.reshape(H, W), ka.rec.reshape(H, W, 4)
    oa[:, 21:23], ra[:, 21:23, 3] = 2, 3.0
    out, src = _run(ka, kb, rec, obj)
    A, B = _img(ka.film["color"]), _img(kb.film["color"])
    assert np.all(src[:, 11:15] == 1)
    assert np.array_equal(_bits(out["color"][:, 11:15]), _bits(A[:, 12:16]))
    assert np.all(src[:, 20:22] == 3)
    assert np.array_equal(_bits(out["color"][:, 20:22]), _bits((f32(0.5) * A[:, 20:22] + f32(0.5) * B[:, 20:22]).astype(f32)))
    # the rest of the interior still blends both keys
    rest = np.ones(W, bool)
    rest[[0, W - 1]] = False
    rest[11:15] = False
    rest[20:22] = False
    assert np.all(src[:, rest] == 0)
    # the same depth with another object, and the same object at another depth, are both rejected
    kb.obj.reshape(H, W)[:, 10:14] = 1
    assert np.all(_run(ka, kb, rec, obj)[1][:, 11:15] == 1)
    kb.rec.reshape(H, W, 4)[:, 10:14, 3] = 4.0
    assert np.all(_run(ka, kb, rec, obj)[1][:, 11:15] == 0)


def test_a_miss_pixel_takes_the_keys_own_pixels():
    """A miss pixel of T looks at the same pixel of each key, which counts when it is a miss too."""
    ka, kb, rec, obj = _case(3)
    obj.reshape(H, W)[:, 5:8] = T.MISS
    rec.reshape(H, W, 4)[:, 5:8] = (0.0, 0.0, 0.0, np.inf)
    ka.obj.reshape(H, W)[:, 5:7] = T.MISS
    kb.obj.reshape(H, W)[:, 6:8] = T.MISS
    out, src = _run(ka, kb, rec, obj)
    A, B = _img(ka.film["color"]), _img(kb.film["color"])
    assert np.all(src[:, 5] == 1) and np.all(src[:, 6] == 0) and np.all(src[:, 7] == 2)
    assert np.array_equal(_bits(out["color"][:, 5]), _bits(A[:, 5])) and np.array_equal(_bits(out["color"][:, 7]), _bits(B[:, 7]))
    assert np.array_equal(_bits(out["color"][:, 6]), _bits((f32(0.5) * A[:, 6] + f32(0.5) * B[:, 6]).astype(f32)))


def test_non_finite_colours_in_the_taps_and_in_the_verbatim_arm():
    ka, kb, rec, obj = _case(4)
    A, B = _img(ka.film["color"]), _img(kb.film["color"])  # views: the edits below reach the keys
    A[3, 9, 1] = np.nan   # the tap of T's (8, 3) in A
    B[4, 9, 0] = np.inf   # the tap of T's (10, 4) in B
    out, src = _run(ka, kb, rec, obj)
    assert src[3, 8] == 2 and np.array_equal(_bits(out["color"][3, 8]), _bits(B[3, 7]))
    assert src[4, 10] == 1 and np.array_equal(_bits(out["color"][4, 10]), _bits(A[4, 11]))
    # tier 2 (both keys occluded for T's column 20): one usable pixel, then none
    kb.obj.reshape(H, W)[:, 19] = 2
    ka.obj.reshape(H, W)[:, 21] = 2
    A[5, 20, 2] = -np.inf
    A[6, 20] = (np.nan, 1.0, 2.0)
    B[6, 20] = (3.0, np.inf, -0.0)
    out, src = _run(ka, kb, rec, obj)
    assert src[4, 20] == 3 and src[5, 20] == 4 and src[6, 20] == 4
    assert np.array_equal(_bits(out["color"][5, 20]), _bits(B[5, 20]))
    assert np.array_equal(_bits(out["color"][6, 20]), _bits(A[6, 20]))  # wA >= wB: A's pixel, non-finite values as they are
    for name in ("alpha", "background", "normal"):
        assert np.array_equal(_bits(out[name][5, 20]), _bits(_img(kb.film[name])[5, 20])), name
        assert np.array_equal(_bits(out[name][6, 20]), _bits(_img(ka.film[name])[6, 20])), name
    assert I.interpolate(W, H, ka, kb, rec, obj, 0.75, [], 0.05)[1].reshape(H, W)[6, 20] == 4
    assert np.array_equal(_bits(_run(ka, kb, rec, obj, ts=0.75)[0]["color"][6, 20]), _bits(B[6, 20]))  # wA < wB: B's


def test_negative_zero_survives_a_single_tap_of_weight_one():
    ka, kb, rec, obj = _case(5)
    A = _img(ka.film["color"])
    A[:, 1] = f32(-0.0)
    out, src = _run(ka, kb, rec, obj)
    assert np.all(src[:, 0] == 1) and np.all(_bits(out["color"][:, 0]) == 0x80000000)


def test_the_depth_test_at_and_one_ulp_beyond_the_tolerance():
    """te = 4 and depth_tolerance = 0.25: a tap at t = 5 is exactly at the bound and counts, the next float does not; likewise below."""
    ka, kb, rec, obj = _case(6)
    r = kb.rec.reshape(H, W, 4)
    r[2, 7, 3] = 5.0
    r[3, 7, 3] = np.nextafter(f32(5.0), f32(np.inf))
    r[4, 7, 3] = 3.0
    r[5, 7, 3] = np.nextafter(f32(3.0), f32(-np.inf))
    r[6, 7, 3] = np.nan
    _, src = _run(ka, kb, rec, obj, tol=0.25)
    assert [int(src[y, 8]) for y in (2, 3, 4, 5, 6)] == [0, 1, 0, 1, 1]
    _, src = _run(ka, kb, rec, obj, tol=0.0)
    assert np.all(src[2:7, 8] == 1) and src[7, 8] == 0


def test_a_generated_frame_at_a_keys_own_time():
    """ts == ta: s = 0, so a pixel both keys see is v_A * 1 + v_B * 0 = v_A; ts == tb likewise.  Sources do not depend on ts here."""
    ka, kb, rec, obj = _case(7)
    A, B = _img(ka.film["color"]), _img(kb.film["color"])
    out, src = _run(ka, kb, rec, obj, ts=0.0)
    assert np.all(src[:, 1:W - 1] == 0) and np.array_equal(out["color"][:, 1:W - 1], A[:, 2:])
    out, src = _run(ka, kb, rec, obj, ts=1.0)
    assert np.all(src[:, 1:W - 1] == 0) and np.array_equal(out["color"][:, 1:W - 1], B[:, :W - 2])


def test_an_animated_hitable_is_moved_to_each_keys_time():
    """Both key cameras and T's are the same; object 1 moves 2 pixels per unit of time along x.  T at 0.5 shows under pixel x what A
    (time 0) shows under x - 1 and B (time 1) under x + 1: P - v * (ts - tK) with the sign as written."""
    ka, kb, rec, obj = _case(8)
    for k in (ka, kb):
        k.camera = T.ortho_camera(W, H, pixel=PIXEL)
        k.rec, k.obj, _ = T.ortho_plane_gbuffer(W, H, pixel=PIXEL)
    out, src = _run(ka, kb, rec, obj, hitables=[(False, (9.0, 9.0, 9.0)), (True, (2 * PIXEL, 0.0, 0.0))])
    A, B = _img(ka.film["color"]), _img(kb.film["color"])
    assert np.all(src[:, 1:W - 1] == 0)
    assert np.array_equal(_bits(out["color"][:, 1:W - 1]), _bits((f32(0.5) * A[:, :W - 2] + f32(0.5) * B[:, 2:]).astype(f32)))
    # not animated: nothing moves
    out, _ = _run(ka, kb, rec, obj, hitables=[(False, (9.0, 9.0, 9.0)), (False, (2 * PIXEL, 0.0, 0.0))])
    assert np.array_equal(_bits(out["color"]), _bits((f32(0.5) * A + f32(0.5) * B).astype(f32)))


def test_fractional_positions_blend_two_taps_per_key():
    """Key cameras half a pixel to each side: fx = x + 0.5 in A, so v_A = (0.5 * A[x] + 0.5 * A[x + 1]) / 1 and v_B from B[x - 1], B[x]."""
    ka, kb, rec, obj = _case(9)
    for k, ox in ((ka, -PIXEL / 2), (kb, PIXEL / 2)):
        k.camera = T.ortho_camera(W, H, origin_x=ox, pixel=PIXEL)
        k.rec, k.obj, _ = T.ortho_plane_gbuffer(W, H, origin_x=ox, pixel=PIXEL)
    out, src = _run(ka, kb, rec, obj, ts=0.25)
    A, B = _img(ka.film["alpha"])[..., 0], _img(kb.film["alpha"])[..., 0]
    h = f32(0.5)
    vA = ((h * A[:, 1:W - 1]).astype(f32) + (h * A[:, 2:]).astype(f32)).astype(f32)
    vB = ((h * B[:, :W - 2]).astype(f32) + (h * B[:, 1:W - 1]).astype(f32)).astype(f32)
    want = ((vA * f32(0.75)).astype(f32) + (vB * f32(0.25)).astype(f32)).astype(f32)
    assert np.all(src[:, 1:W - 1] == 0) and np.array_equal(_bits(out["alpha"][:, 1:W - 1, 0]), _bits(want))
    # at the border one tap of the pair is outside: the other alone, renormalised
    assert np.all(src[:, 0] == 0) and np.array_equal(_bits(out["alpha"][:, 0, 0]), _bits((((h * A[:, 0]).astype(f32) + (h * A[:, 1]).astype(f32)).astype(f32) * f32(0.75)
                                                                                            + ((h * B[:, 0]).astype(f32) / h).astype(f32) * f32(0.25)).astype(f32)))


# ---- the option, the plan and the keys ---------------------------------------------------------------------------------------------------

def test_interpolate_validation():
    import rayn_amd as R
    assert (R.Interpolate().every, R.Interpolate().depth_tolerance) == (2, 0.25)
    assert R.Interpolate(16, 0.0).to_abi().depth_tolerance == 0.0
    for bad in (1, 17, 0, -2, 2.0, True, "2", None):
        with pytest.raises(ValueError, match="Interpolate.every"):
            R.Interpolate(bad)
    for bad in (-0.1, float("nan"), float("inf"), 1e39, "x", None, True):
        with pytest.raises(ValueError, match="Interpolate.depth_tolerance"):
            R.Interpolate(2, bad)


@pytest.mark.parametrize("k", [2, 3, 4])
def test_which_entries_are_keys(k):
    """Entry i is a key when i % k == 0 or it is the last entry, for lists of 1, 2, k, k + 1 and 2k + 1 frames."""
    import rayn_amd as R
    it = R.Interpolate(k)
    for n in (1, 2, k, k + 1, 2 * k + 1):
        got = [i for i in range(n) if it.is_key(i, n)]
        assert got == sorted(set(range(0, n, k)) | {n - 1}), (k, n)
        assert got[0] == 0 and got[-1] == n - 1 and all(b - a <= k for a, b in zip(got, got[1:]))
    assert [i for i in range(2 * k + 1) if it.is_key(i, 2 * k + 1)] == [0, k, 2 * k]
    assert [i for i in range(k + 1) if it.is_key(i, k + 1)] == [0, k]
    assert [i for i in range(k) if it.is_key(i, k)] == [0, k - 1]


def test_plan_sequence_rules_and_file_names():
    import rayn_amd as R
    from rayn_amd.film import plan_sequence
    K = R.ChannelKind
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    it = R.Interpolate(3)
    plan = plan_sequence(kinds, [K.Color, K.Alpha], interpolate=it)
    assert plan.interpolate is it and plan.interp_keys == ["color", "alpha", "background", "normal"]
    assert [s for _, _, s in plan.jobs] == ["color_interp", "alpha"]
    plan = plan_sequence([K.Color, K.WorldNormal], [K.Color, K.WorldNormal], denoise=R.Denoise(), display=R.Display(), interpolate=it)
    assert [s for _, _, s in plan.jobs] == ["color_interp_denoised_display", "normal"] and plan.interp_keys == ["color", "normal"]
    assert [s for _, _, s in plan_sequence(kinds, [K.Alpha], interpolate=it).jobs] == ["alpha"]
    none = plan_sequence(kinds, [K.Color], interpolate=None)
    assert none.interpolate is None and none.interp_keys is None and [s for _, _, s in none.jobs] == ["color"]
    for kw in (dict(temporal=R.Temporal()), dict(upscale=R.Upscale()), dict(upscale=R.Upscale(), temporal=R.Temporal(), supersample=R.Supersample()),
               dict(preview=R.Preview())):
        with pytest.raises(ValueError, match="not built"):
            plan_sequence(kinds, [K.Color], interpolate=it, **kw)
    with pytest.raises(ValueError, match="must be an Interpolate"):
        plan_sequence(kinds, [K.Color], interpolate=2)
    with pytest.raises(ValueError, match="without a Color channel"):
        plan_sequence([K.Alpha], [K.Alpha], interpolate=it)
    with pytest.raises(ValueError, match="VarianceDenoise"):
        plan_sequence(kinds, [K.Color], denoise=R.VarianceDenoise(), interpolate=it)


def test_render_sequence_rejects_before_anything_renders(tmp_path):
    """The rules need nothing of the film: a bare Film raises them, and no directory appears."""
    import rayn_amd as R
    K = R.ChannelKind
    film = R.Film.__new__(R.Film)
    film.channel_kinds = [K.Color, K.WorldNormal]
    with pytest.raises(ValueError, match="not built"):
        film.render_sequence(None, None, None, None, (16, 16), [1, 2, 3], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "x"), "a", temporal=R.Temporal(),
                             interpolate=R.Interpolate())
    assert not (tmp_path / "x").exists()
