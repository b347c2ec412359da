"""The temporal accumulation on the CPU: properties of its numpy restatement (tests/temporal_np.py) - static reprojection, the running mean,
a known camera translation, every rejection rule, the quarantine of a non-finite colour - the host-only size functions of the library and the
validation of rayn_amd.Temporal.  tests/test_temporal_device.py holds the GPU kernels to the same restatement bit for bit."""
import numpy as np
import pytest

import temporal_np as T
from common import case

f32 = np.float32
W, H = 16, 8  # powers of two: the synthetic orthographic case is exact
NOHIT = []    # no animated hitables


def _colors(k, seed=0):
    return np.random.default_rng(seed).gamma(0.6, 0.5, (k, W * H, 3)).astype(f32)


def _acc(color, normal, rec, obj, prev, cam, **kw):
    args = dict(max_history=32, depth_tolerance=0.05, normal_min=0.9)
    args.update(kw)
    return T.accumulate(W, H, color, normal, rec, obj, prev, cam, 0.0, 0.0, NOHIT, want_taps=True, **args)


def test_static_camera_reprojects_every_hit_pixel_onto_itself(oracle):
    """The shipped scene through the oracle's camera and closest hit: with nothing moving, every hit pixel's taps sum to weight 1 (up to the
    f32 rounding of the projection, which may put 1e-5 of it on a neighbour that fails a test) and the history length becomes 2."""
    wd, p = case("s2", 48, 32, 2, 3)
    rec, obj = T.gbuffer_oracle(oracle, wd, p)
    rng = np.random.default_rng(1)
    color, normal = rng.random((48 * 32, 3)).astype(f32), rng.normal(size=(48 * 32, 3)).astype(f32)
    hit = obj != T.MISS
    assert hit.sum() > 1000
    _, hist = T.accumulate(48, 32, color, normal, rec, obj, None, None, 0.0, p.time_start, T.world_hitables(wd), 32, 0.05, -1.0)
    assert np.all(hist[0][:, 3] == 1.0) and np.array_equal(hist[0][:, :3], color) and np.array_equal(hist[1], rec)
    out, hist2, Wt = T.accumulate(48, 32, color, normal, rec, obj, hist, wd.camera, p.time_start, p.time_start, T.world_hitables(wd), 32, 0.05, -1.0,
                                  want_taps=True)
    assert np.all(np.abs(Wt[hit] - 1.0) < 1e-4), np.abs(Wt[hit] - 1.0).max()
    assert np.all(hist2[0][hit, 3] == 2.0) and np.all(hist2[0][~hit, 3] == 1.0)
    assert np.array_equal(out[~hit], color[~hit])  # a miss resets


def test_history_length_and_running_mean():
    """k frames of identical geometry: n = min(k, max_history) and out follows out = h + (c - h) / n' in f32 exactly."""
    cam = T.ortho_camera(W, H)
    rec, obj, normal = T.ortho_plane_gbuffer(W, H)
    cs = _colors(7)
    for max_history in (1, 3, 32):
        prev, mean = None, None
        for k, c in enumerate(cs, 1):
            out, prev, Wt = _acc(c, normal, rec, obj, prev, cam, max_history=max_history)
            n = min(k, max_history)
            mean = c if k == 1 else (mean + (f32(1.0) / f32(n) * (c - mean).astype(f32)).astype(f32)).astype(f32)
            assert np.all(prev[0][:, 3] == n), (k, max_history)
            assert np.array_equal(out.view(np.uint32), mean.view(np.uint32)), (k, max_history)
            assert k == 1 or np.all(Wt == 1.0)
    # with max_history = 1 the output is the frame itself, up to the rounding of h + (c - h)
    h0 = cs[0]
    out1, _, _ = _acc(cs[1], normal, rec, obj, _acc(h0, normal, rec, obj, None, cam)[1], cam, max_history=1)
    assert np.array_equal(out1, (h0 + (cs[1] - h0).astype(f32)).astype(f32)) and np.allclose(out1, cs[1], rtol=1e-5, atol=1e-6)


def test_known_camera_translation_lands_on_the_known_pixel():
    """The previous camera stood 3 pixels (and then 2.25 pixels) to the left: current pixel x shows what previous pixel x + 3 showed, and
    x + 2.25 is the bilinear mix 0.75 / 0.25 of x + 2 and x + 3."""
    rec, obj, normal = T.ortho_plane_gbuffer(W, H)
    c0, c1 = _colors(2, 5)
    for shift, taps in ((3.0, {3: 1.0}), (2.25, {2: 0.75, 3: 0.25})):
        prev_cam = T.ortho_camera(W, H, origin_x=-shift * 0.125)
        prev_rec, prev_obj, _ = T.ortho_plane_gbuffer(W, H, origin_x=-shift * 0.125)
        _, prev, _ = _acc(c0, normal, prev_rec, prev_obj, None, None)
        ok, fx, fy, te = T.project(prev_cam, 0.0, [rec[:, 0], rec[:, 1], rec[:, 2]], W, H)
        xs, ys = np.arange(W * H) % W, np.arange(W * H) // W
        assert ok.all() and np.array_equal(fx, (xs + shift).astype(f32)) and np.array_equal(fy, ys.astype(f32)) and np.all(te == 4.0)
        out, hist, Wt = _acc(c1, normal, rec, obj, prev, prev_cam)
        img0, img1, o = c0.reshape(H, W, 3), c1.reshape(H, W, 3), out.reshape(H, W, 3)
        lo, hi = min(taps), max(taps)
        inside = W - hi  # columns whose taps all lie inside the previous image
        h = sum(f32(w) * img0[:, d:d + inside] for d, w in taps.items()).astype(f32)
        want = (h + (f32(0.5) * (img1[:, :inside] - h).astype(f32)).astype(f32)).astype(f32)
        assert np.array_equal(o[:, :inside], want)
        assert np.all(Wt.reshape(H, W)[:, :inside] == 1.0) and np.all(hist[0].reshape(H, W, 4)[:, :inside, 3] == 2.0)
        # columns whose every tap is outside the previous image reset
        assert np.array_equal(o[:, W - lo:], img1[:, W - lo:]) and np.all(hist[0].reshape(H, W, 4)[:, W - lo:, 3] == 1.0)


def _one_frame_history(seed=7):
    cam = T.ortho_camera(W, H)
    rec, obj, normal = T.ortho_plane_gbuffer(W, H)
    c0, c1 = _colors(2, seed)
    _, prev, _ = _acc(c0, normal, rec, obj, None, None)
    return cam, rec, obj, normal, c1, [a.copy() for a in prev]


@pytest.mark.parametrize("rule", ["object", "depth", "normal", "behind", "outside", "nan colour", "no history length"])
def test_every_rejection_rule_resets_the_pixel(rule):
    cam, rec, obj, normal, c1, prev = _one_frame_history()
    j = 3 + 2 * W  # the pixel under test; every other pixel must still blend
    kw = {}
    if rule == "object":
        prev[3][j] = 5
    elif rule == "depth":
        prev[1][j, 3] = 4.0 * 1.06  # 6 % off at a tolerance of 5 %
    elif rule == "normal":
        prev[2][j, :3] = (0.0, 0.6, 0.8)  # dot 0.8 < 0.9
    elif rule == "behind":
        rec = rec.copy()
        rec[j, 2] = 5.0  # behind the orthographic camera's plane z = 4: te = -1
    elif rule == "outside":
        rec = rec.copy()
        rec[j, 0] = 100.0
    elif rule == "nan colour":
        c1 = c1.copy()
        c1[j, 1] = np.nan
    else:
        prev[0][j, 3] = 0.0
    out, hist, Wt = _acc(c1, normal, rec, obj, prev, cam, **kw)
    others = np.arange(W * H) != j
    assert np.all(hist[0][others, 3] == 2.0) and np.all(Wt[others] == 1.0)
    assert Wt[j] == 0.0
    assert np.array_equal(out[j].view(np.uint32), c1[j].view(np.uint32))
    assert hist[0][j, 3] == (0.0 if rule == "nan colour" else 1.0)
    # the depth and normal tests can be switched off, and then the pixel blends again
    if rule == "depth":
        assert _acc(c1, normal, rec, obj, prev, cam, depth_tolerance=0.07)[1][0][j, 3] == 2.0
    if rule == "normal":
        assert _acc(c1, normal, rec, obj, prev, cam, normal_min=-1.0)[1][0][j, 3] == 2.0
        assert _acc(c1, normal, rec, obj, prev, cam, normal_min=0.8)[1][0][j, 3] == 2.0  # a dot product equal to the floor counts
    if rule == "behind":  # the pinhole's rule: a point behind the camera (zc <= 0)
        pin = T.ortho_camera(W, H)
        pin.kind, pin.vfov_or_size = 0, 60.0
        ok, _, _, _ = T.project(pin, 0.0, [np.array([0.0, 0.0], f32), np.array([0.0, 0.0], f32), np.array([0.0, 5.0], f32)], W, H)
        assert ok.tolist() == [True, False]


def test_a_non_finite_colour_never_becomes_a_tap():
    """Frame 2 has an inf at pixel j: it passes through with n' = 0.  In frame 3 the camera has moved half a pixel, so j is a tap of two
    pixels: they take their other tap alone (weight 0.5, renormalised), stay finite, and nothing of the inf spreads."""
    cam, rec, obj, normal, c1, prev = _one_frame_history(11)
    j = 5 + 3 * W
    c1 = c1.copy()
    c1[j] = (np.inf, 1.0, 2.0)
    out, hist, _ = _acc(c1, normal, rec, obj, prev, cam)
    assert hist[0][j, 3] == 0.0 and np.isinf(out[j, 0])
    rec3, obj3, _ = T.ortho_plane_gbuffer(W, H, origin_x=0.0625)
    c2 = _colors(1, 13)[0]
    out3, hist3, Wt = _acc(c2, normal, rec3, obj3, hist, cam)
    assert np.isfinite(out3).all() and np.isfinite(hist3[0]).all()
    wt = Wt.reshape(H, W)
    assert wt[3, 4] == 0.5 and wt[3, 5] == 0.5 and wt[3, 3] == 1.0
    h = hist[0][j - 1, :3]  # pixel (4, 3) sees taps (4, 3) and (5, 3): only the first counts
    n1 = f32(hist[0][j - 1, 3] + f32(1.0))
    want = (h + (f32(1.0) / n1 * (c2[j - 1] - h).astype(f32)).astype(f32)).astype(f32)
    assert np.array_equal(out3[j - 1], want)


def test_object_motion_is_taken_out_before_the_projection():
    """An animated hitable that moved one pixel to the right between the frames: its points are shifted back by center_vel * dt and land on
    the pixel that showed them; a hitable that is not animated is not shifted."""
    cam = T.ortho_camera(W, H)
    rec0, obj, normal = T.ortho_plane_gbuffer(W, H)
    rec1, _, _ = T.ortho_plane_gbuffer(W, H, origin_x=0.125)  # the same surface points, one pixel further right
    c0, c1 = _colors(2, 17)
    _, prev, _ = _acc(c0, normal, rec0, obj, None, None)
    moving = [(False, (0.0, 0.0, 0.0)), (True, (0.25, 0.0, 0.0))]  # object 1: 0.25 units per time unit, dt = 0.5
    out, hist, Wt = T.accumulate(W, H, c1, normal, rec1, obj, prev, cam, 1.0, 1.5, moving, 32, 0.05, 0.9, want_taps=True)
    assert np.all(Wt == 1.0) and np.all(hist[0][:, 3] == 2.0)
    want = (c0 + (f32(0.5) * (c1 - c0).astype(f32)).astype(f32)).astype(f32)
    assert np.array_equal(out, want)
    still = [(False, (0.0, 0.0, 0.0)), (False, (0.25, 0.0, 0.0))]
    _, hist, _ = T.accumulate(W, H, c1, normal, rec1, obj, prev, cam, 1.0, 1.5, still, 32, 0.05, 0.9, want_taps=True)
    assert np.all(hist[0].reshape(H, W, 4)[:, -1, 3] == 1.0)  # the last column now looks outside the previous image


def test_gbuffer_assembly():
    org = np.array([[1.0, 2.0, 3.0], [0.0, 0.0, 0.0]], f32)
    d = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.0]], f32)
    rec, obj = T.gbuffer_assemble(org, d, np.array([2.5, 7.0], f32), np.array([3, 0xFFFFFFFF], np.uint32))
    assert np.array_equal(rec[0], np.array([f32(1.0) + f32(2.5) * f32(0.1), f32(2.0) + f32(2.5) * f32(0.2), f32(3.0) + f32(2.5) * f32(0.3), 2.5], f32))
    assert rec[1].tolist() == [0.0, 0.0, 0.0, np.inf] and obj.tolist() == [3, 0xFFFFFFFF]


def test_host_only_size_functions():
    from rayn_amd import film as F
    for w, h in [(1, 1), (48, 32), (40, 24), (50, 37), (1920, 1080), (65536, 32767)]:
        npad = (w * h + 63) // 64 * 64
        assert F.gbuffer_scratch_bytes(w, h) == 53 * npad + 384, (w, h)
        assert F.temporal_history_bytes(w, h) == 52 * w * h, (w, h)
    for w, h in [(0, 5), (5, 0), (65536, 32768), (0xFFFFFFFF, 0xFFFFFFFF)]:  # zero-sized, and width * height >= 2^31
        assert F.gbuffer_scratch_bytes(w, h) == 0 and F.temporal_history_bytes(w, h) == 0, (w, h)
    n = 6
    A, B, N, O = np.arange(4 * n, dtype=f32).reshape(n, 4), np.ones((n, 4), f32), np.zeros((n, 4), f32), np.arange(n, dtype=np.uint32)
    back = T.split_history(T.join_history(A, B, N, O), n)
    assert all(np.array_equal(x, y) for x, y in zip(back, (A, B, N, O))) and T.join_history(A, B, N, O).size == 52 * n


def test_temporal_validation():
    import rayn_amd as R
    t = R.Temporal()
    assert (t.max_history, t.depth_tolerance, t.normal_min) == (4, 0.05, -1.0)
    a = R.Temporal(max_history=65536, depth_tolerance=0, normal_min=1).to_abi()
    assert (a.max_history, a.depth_tolerance, a.normal_min) == (65536, 0.0, 1.0)
    for bad in (dict(max_history=0), dict(max_history=65537), dict(max_history=2.0), dict(max_history=True), dict(depth_tolerance=-0.1),
                dict(depth_tolerance=float("inf")), dict(depth_tolerance=float("nan")), dict(depth_tolerance=1e39), dict(depth_tolerance="x"),
                dict(normal_min=-1.5), dict(normal_min=1.01), dict(normal_min=float("nan")), dict(normal_min=None)):
        with pytest.raises(ValueError, match="Temporal"):
            R.Temporal(**bad)
    import dataclasses
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.max_history = 3


def test_render_sequence_rejects_a_bad_temporal_before_anything_runs():
    """render_sequence checks `temporal` before it touches the GPU (no film is created here: Film() needs one)."""
    import inspect
    import rayn_amd as R
    sig = inspect.signature(R.Film.render_sequence)
    assert sig.parameters["temporal"].default is None and list(sig.parameters)[-1] == "temporal"
