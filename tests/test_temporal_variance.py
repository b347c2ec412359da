"""Properties of the numpy restatement of the luminance moments and of the variance estimate of a temporally accumulated colour
(tests/temporal_variance_np.py) on hand-made inputs, the size helper, and the argument rule of Film.render_sequence.  No GPU;
tests/test_temporal_variance_device.py holds the kernels to the restatement bit for bit."""
import numpy as np
import pytest

import temporal_np as T
import temporal_variance_np as TV

f32 = np.float32


def _run(w, h, colours, shift_px=0.0, max_history=4):
    """A sequence over the plane z = 0 under the exact orthographic camera, the camera moving right by shift_px pixels per frame;
    colours[i]: (n, 3) or one colour.  Returns the list of (out, history, moments) per frame."""
    res, prev, mom, prev_cam = [], None, None, None
    for i, c in enumerate(colours):
        ox = i * shift_px * 0.125
        rec, obj, normal = T.ortho_plane_gbuffer(w, h, origin_x=ox)
        color = np.broadcast_to(np.asarray(c, f32), (w * h, 3)).copy()
        out, prev, mom = TV.accumulate(w, h, color, normal, rec, obj, prev, mom, prev_cam, 0.0, 0.0, [], max_history, 0.05, -1.0)
        prev_cam = T.ortho_camera(w, h, origin_x=ox)
        res.append((out, prev, mom))
    return res


def test_a_constant_luminance_keeps_its_moments_and_has_no_variance():
    w, h = 16, 8
    c = (0.7, 0.2, 0.4)
    res = _run(w, h, [c] * 5)
    y = TV.luminance(np.array([c], f32))[0]
    for i, (out, hist, mom) in enumerate(res):
        assert np.all(mom[:, 0] == y) and np.all(mom[:, 1] == f32(y * y)), i
        assert np.all(hist[0][:, 3] == min(i + 1, 4))
    out, hist, mom = res[-1]
    v, _ = TV.initial_variance(w, h, out, hist[3], hist[0][:, 3], mom)  # n' = 4: the temporal estimate, m2 - m1 * m1 = 0 exactly
    assert np.all(v == 0.0)
    out, hist, mom = res[1]
    v, k = TV.initial_variance(w, h, out, hist[3], hist[0][:, 3], mom)  # n' = 2: the spatial one, zero up to the rounding of its sums
    assert np.all(np.isfinite(v)) and v.max() <= 1e-5 * y * y and k.max() == 49 and k.min() == 16


def _by_hand(ys, max_history):
    """The moments of a pixel that saw the luminances ys, oldest first, each reprojected with full weight"""
    m1, m2 = f32(ys[0]), f32(f32(ys[0]) * f32(ys[0]))
    for j, y in enumerate(ys[1:], 1):
        y = f32(y)
        a = f32(f32(1.0) / f32(min(j + 1, max_history)))
        m1 = f32(m1 + f32(a * f32(y - m1)))
        m2 = f32(m2 + f32(a * f32(f32(y * y) - m2)))
    return m1, m2


@pytest.mark.parametrize("max_history", [2, 4, 16])
def test_a_two_valued_sequence_reproduces_the_moments_computed_by_hand(max_history):
    """The camera moves one whole pixel per frame, so every tap has weight 1 or 0 and the history of column x is as long as the number of
    frames that column has been inside the image: the column that enters resets, the others blend the two values in turn."""
    w, h, frames = 16, 8, 6
    ca, cb = (0.9, 0.5, 0.1), (0.1, 0.3, 0.8)
    cols = [ca if i % 2 == 0 else cb for i in range(frames)]
    ys = [TV.luminance(np.array([c], f32))[0] for c in cols]
    res = _run(w, h, cols, shift_px=1.0, max_history=max_history)
    for i, (out, hist, mom) in enumerate(res):
        m = mom.reshape(h, w, 2)
        n1 = hist[0][:, 3].reshape(h, w)
        for x in range(w):
            length = min(i, w - 1 - x) + 1  # frames this world column has been seen
            m1, m2 = _by_hand(ys[i + 1 - length: i + 1], max_history)
            assert np.all(m[:, x, 0] == m1) and np.all(m[:, x, 1] == m2), (i, x)
            assert np.all(n1[:, x] == min(length, max_history))
    # the variance of the mean at a long history: (m2 - m1^2) / n'
    out, hist, mom = res[-1]
    v, _ = TV.initial_variance(w, h, out, hist[3], hist[0][:, 3], mom)
    long = hist[0][:, 3] >= 4
    assert long.any() == (max_history >= 4)
    d = (mom[:, 1] - (mom[:, 0] * mom[:, 0]).astype(f32)).astype(f32)
    assert np.array_equal(v[long], (np.maximum(d, f32(0.0)) / hist[0][:, 3])[long])


def test_a_checkerboard_under_the_spatial_estimate_has_the_closed_form_variance():
    w, h = 20, 14
    xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    odd = ((xs + ys) % 2).reshape(-1).astype(bool)
    a, b = f32(0.25), f32(0.75)
    color = np.where(odd[:, None], b, a).astype(f32) * np.ones((1, 3), f32)
    la, lb = TV.luminance(np.array([[a] * 3], f32))[0], TV.luminance(np.array([[b] * 3], f32))[0]
    obj = np.ones(w * h, np.uint32)
    v, k = TV.initial_variance(w, h, color, obj, np.full(w * h, 2.0, f32), np.zeros((w * h, 2), f32))
    v, k = v.reshape(h, w), k.reshape(h, w)
    assert np.all(k[3:-3, 3:-3] == 49)
    # 25 taps of the centre's value and 24 of the other: variance 25 * 24 / 49^2 (la - lb)^2
    want = 25.0 * 24.0 / 49.0 ** 2 * (float(la) - float(lb)) ** 2
    assert np.allclose(v[3:-3, 3:-3], want, rtol=2e-5, atol=0.0)
    # with n' >= 4 the window is not looked at
    m = np.stack([np.full(w * h, 0.5, f32), np.full(w * h, 0.375, f32)], axis=1)
    vt, _ = TV.initial_variance(w, h, color, obj, np.full(w * h, 4.0, f32), m)
    assert np.all(vt == f32(0.125) / f32(4.0))


def test_the_window_is_clipped_by_the_image_and_by_objects_and_skips_what_is_no_tap():
    w, h = 12, 10
    rng = np.random.default_rng(1)
    color = rng.random((w * h, 3)).astype(f32)
    obj = np.ones((h, w), np.uint32)
    obj[:, 7:] = 2             # an object boundary between columns 6 and 7
    obj[9, 0] = T.MISS         # a miss
    n1 = np.full((h, w), 1.0, f32)
    n1[5, 5] = 0.0             # no history and no estimate: not a tap
    color.reshape(h, w, 3)[4, 4, 1] = np.inf  # a colour that is not finite: not a tap
    v, k = TV.initial_variance(w, h, color, obj.reshape(-1), n1.reshape(-1), np.zeros((w * h, 2), f32))
    v, k = v.reshape(h, w), k.reshape(h, w)
    assert k[0, 0] == 16 and k[0, 3] == 7 * 4          # the image corner and the bottom edge
    assert k[0, 11] == 4 * 4 and k[0, 8] == 5 * 4      # object 2: columns 7..11
    assert k[0, 6] == 4 * 4                            # object 1 at column 6: columns 3..6 of rows 0..3
    assert k[7, 3] == 6 * 7 - 3                        # rows 4..9, columns 0..6, minus (4, 4), (5, 5) and the miss at (9, 0)
    assert np.isnan(v[9, 0]) and np.isnan(v[5, 5]) and np.isnan(v[4, 4])
    assert np.isfinite(np.delete(v.reshape(-1), [9 * w, 5 * w + 5, 4 * w + 4])).all()


def test_temporal_moments_bytes():
    from rayn_amd import _abi
    from rayn_amd import film as F
    for w, h in [(1, 1), (37, 23), (160, 96), (1920, 1080), (0, 5), (5, 0), (65536, 32768), (46341, 46341)]:
        want = 8 * w * h if F.temporal_history_bytes(w, h) else 0
        assert F.temporal_moments_bytes(w, h) == want == _abi.temporal_moments_bytes(w, h) == TV.moments_bytes(w, h), (w, h)
    assert F.temporal_moments_bytes(37, 23) == 8 * 37 * 23 and F.temporal_moments_bytes(65536, 32768) == 0


def test_render_sequence_with_a_variance_denoiser_and_no_temporal_still_raises_before_anything_runs(tmp_path):
    """The film is never rendered (there may be no GPU): the argument check comes first and nothing is written."""
    import os
    import rayn_amd as R
    K = R.ChannelKind
    film = R.Film.__new__(R.Film)  # no context: the check must not need one
    with pytest.raises(ValueError, match="render_sequence renders plain frames: VarianceDenoise needs the state of a progressive render"):
        film.render_sequence(None, None, None, None, (16, 16), [1], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "seq"), "a", denoise=R.VarianceDenoise())
    assert not os.path.exists(tmp_path / "seq")
