"""rayn_hip_interpolate_device (rayn_amd/csrc/interpolate.hip) on the GPU: the kernel bit for bit against its numpy restatement
(tests/interpolate_np.py) on the synthetic cases of tests/test_interpolate.py, on adversarial random inputs and on rendered keys of moving
scenes under the three cameras and both mul_add policies; input hygiene and every error text; Film.render_sequence(interpolate=...) against
the plain sequence and the loop of the entries; Film.interpolated; and the quality of a generated frame against the plain cross-fade."""
import ctypes as C
import os

import numpy as np
import pytest

import device_io as IO
import interpolate_np as I
import scenes
import temporal_np as T
from common import bits_equal
from device_io import module_context as ctx  # noqa: F401
from temporal_cases import SIZES, SPECIAL

pytestmark = pytest.mark.gpu

f32 = np.float32
PLANE_FLOATS = {"color": 3, "alpha": 1, "background": 3, "normal": 3}


def _gpu_interpolate(ctx, w, h, ka, kb, rec, obj, ts, tol, guard=64, source=True):
    """The entry through Context.interpolate on host arrays -> ({plane: (n, c)}, source (n,) uint32 or None).  Checks the guard floats
    behind every output, that no input changed and that an absent plane's output stays untouched."""
    import torch
    import rayn_amd as R
    n = w * h
    p = R.frame_params(w, h, 1, 1, time_range=(float(ts), float(ts) + 0.04))
    dev = [(IO.upload_film(k.film), IO.upload_gbuffer(k.rec, k.obj)) for k in (ka, kb)]
    g = IO.upload_gbuffer(rec, obj)
    ins = [t for f, gk in dev + [({}, g)] for t in (*f.values(), *gk.values())]
    keep = IO.snapshot(ins)
    full = {k: IO.guarded(c * n, torch.float32, 7.0, guard) for k, c in PLANE_FLOATS.items()}
    d_out = {k: full[k][1] for k in dev[0][0]}
    full_src, d_src = IO.guarded(n, torch.int32, -3, guard)
    ctx.interpolate(p, R.Interpolate(2, tol), (dev[0][0], dev[0][1], ka.camera, ka.time), (dev[1][0], dev[1][1], kb.camera, kb.time), g, d_out,
                    d_src if source else None)
    torch.cuda.synchronize()
    for k, c in PLANE_FLOATS.items():
        IO.assert_guards(full[k][0], c * n if k in d_out else 0, 7.0, k)
    IO.assert_guards(full_src, n if source else 0, -3, "d_out_source")
    IO.assert_unchanged(ins, keep, "a key or the G-buffer")
    out = {k: d_out[k].cpu().numpy().reshape(n, PLANE_FLOATS[k]) for k in d_out}
    return out, (d_src.cpu().numpy().view(np.uint32) if source else None)


def _same(got, want, what):
    (out_g, src_g), (out_w, src_w) = got, want
    if src_g is not None:
        assert np.array_equal(src_g, src_w), (what, "source", int((src_g != src_w).sum()))
    IO.assert_planes_equal(out_g, out_w, what)


def _check(ctx, w, h, ka, kb, rec, obj, ts, tol, hitables, what, **kw):
    want = I.interpolate(w, h, ka, kb, rec, obj, ts, hitables, tol)
    _same(_gpu_interpolate(ctx, w, h, ka, kb, rec, obj, ts, tol, **kw), want, what)
    return want


# ---- 1. the synthetic cases ---------------------------------------------------------------------------------------------------------------

def test_kernel_on_the_exact_orthographic_cases(ctx):
    """The cases tests/test_interpolate.py writes down pixel by pixel, through the kernel: both keys, one key, tier 2, special values, the
    depth bound, ts at either key, a moving hitable, fractional positions, absent planes - and every source code occurs."""
    W, H, PIXEL = 32, 16, 0.125
    wd, _, _ = scenes.scene("s0", (W, H))
    ctx.upload_world(wd)  # no animated hitable
    seen = set()
    ka, kb, rec, obj = I.ortho_case(W, H, 2, PIXEL)
    for key, cols in ((kb, slice(10, 14)), (kb, slice(19, 21)), (ka, slice(21, 23))):
        key.obj.reshape(H, W)[:, cols], key.rec.reshape(H, W, 4)[:, cols, 3] = 2, 3.0
    A, B = ka.film["color"].reshape(H, W, 3), kb.film["color"].reshape(H, W, 3)
    A[3, 9, 1], B[4, 9, 0], A[5, 20, 2] = np.nan, np.inf, -np.inf
    A[6, 20], B[6, 20] = (np.nan, 1.0, 2.0), (3.0, np.inf, -0.0)
    A[:, 1] = f32(-0.0)
    obj.reshape(H, W)[:, 5:8] = T.MISS
    rec.reshape(H, W, 4)[:, 5:8] = (0.0, 0.0, 0.0, np.inf)
    ka.obj.reshape(H, W)[:, 5:7] = T.MISS
    kb.obj.reshape(H, W)[:, 6:8] = T.MISS
    r = kb.rec.reshape(H, W, 4)
    r[2, 25, 3], r[3, 25, 3], r[4, 25, 3], r[5, 25, 3], r[6, 25, 3] = 5.0, np.nextafter(f32(5.0), f32(np.inf)), 3.0, np.nextafter(f32(3.0), f32(-np.inf)), np.nan
    for ts in (0.5, 0.0, 1.0, 0.75, 0.3):
        for tol in (0.25, 0.05, 0.0):
            _, src = _check(ctx, W, H, ka, kb, rec, obj, ts, tol, [], ("ortho", ts, tol))
            seen |= set(np.unique(src).tolist())
    assert [int(I.interpolate(W, H, ka, kb, rec, obj, 0.5, [], 0.25)[1].reshape(H, W)[y, 26]) for y in (2, 3, 4, 5, 6)] == [0, 1, 0, 1, 1]
    assert seen == {0, 1, 2, 3, 4}
    # absent planes are neither read nor written; no source plane
    whole = [dict(k.film) for k in (ka, kb)]
    for planes in (("color",), ("color", "normal"), ("color", "alpha", "background")):
        for k, film in zip((ka, kb), whole):
            k.film = {p: v for p, v in film.items() if p in planes}
        _check(ctx, W, H, ka, kb, rec, obj, 0.5, 0.05, [], ("planes", planes), source=len(planes) != 2)
    # fractional positions
    ka, kb, rec, obj = I.ortho_case(W, H, 9, PIXEL)
    for k, ox in ((ka, -PIXEL / 2), (kb, PIXEL / 4)):
        k.camera = T.ortho_camera(W, H, origin_x=ox, pixel=PIXEL)
        k.camera.origin.y = k.camera.at.y = ox / 2
        k.rec, k.obj, _ = T.ortho_plane_gbuffer(W, H, origin_x=ox, pixel=PIXEL)
    _check(ctx, W, H, ka, kb, rec, obj, 0.25, 0.05, [], "fractional")
    # a moving hitable: the world's animated fractal is object 1
    wd, _, _ = scenes.scene("s1", (W, H), moving=True)
    ctx.upload_world(wd)
    hit = T.world_hitables(wd)
    assert hit[1][0]
    ka, kb, rec, obj = I.ortho_case(W, H, 8, PIXEL)
    want = _check(ctx, W, H, ka, kb, rec, obj, 0.5, 0.05, hit, "moving")
    still = I.interpolate(W, H, ka, kb, rec, obj, 0.5, [], 0.05)
    assert not np.array_equal(want[1], still[1]) or not bits_equal(want[0]["color"], still[0]["color"])


# ---- 2. adversarial random inputs ---------------------------------------------------------------------------------------------------------

def _random_case(w, h, seed, cam_kind, adversarial):
    """Two keys and a frame around the plane z = 0 under three different cameras, with random objects, misses, depths scattered around what
    each projection expects and random planes; `adversarial` scatters NaN / inf / huge values over the colours and the records."""
    from rayn_amd import _abi
    rng = np.random.default_rng(seed)
    n = w * h
    cams = []
    for k in range(2):
        c = T.ortho_camera(w, h, origin_x=float(rng.uniform(-0.6, 0.6)), pixel=4.0 / h)
        c.origin.y = c.at.y = float(rng.uniform(-0.5, 0.5))
        if cam_kind != _abi.CAM_ORTHOGRAPHIC:
            c.kind, c.vfov_or_size = cam_kind, 53.0
            c.at.x += 0.3 * (k - 0.5)
            c.animated, c.origin_vel.z, c.up_vel.x = 1 | 4, 0.5, 0.2
        cams.append(c)
    rec, obj, _ = T.ortho_plane_gbuffer(w, h, pixel=4.0 / h)
    rec[:, 2] = rng.normal(0.0, 0.05, n)
    choices = np.array([0, 1, 1, 1, 2, 0xFFFFFFFF], np.uint32)
    obj = rng.choice(choices, n)
    rec[obj == T.MISS] = (0.0, 0.0, 0.0, np.inf)
    ta, tb = 0.25, 0.75
    keys = []
    for c, t in zip(cams, (ta, tb)):
        ok, fx, fy, te = T.project(c, t, [rec[:, 0], rec[:, 1], rec[:, 2]], w, h)
        depth = (np.nanmedian(te[ok]) if ok.any() else 4.0) * rng.choice(np.array([1.0, 1.0, 1.02, 0.97, 1.2]), n)
        krec = np.concatenate([rng.normal(size=(n, 3)), depth[:, None]], axis=1).astype(f32)
        kobj = rng.choice(choices, n)
        film = {"color": rng.gamma(0.6, 0.5, (n, 3)).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
                "normal": rng.normal(size=(n, 3)).astype(f32)}
        if adversarial:
            for plane in (film["color"], krec, rec):
                flat = plane.reshape(-1)
                idx = rng.choice(flat.size, min(flat.size // 4, 6 * SPECIAL.size), replace=False)
                flat[idx] = np.resize(SPECIAL, idx.size)
        keys.append(I.Key(film, krec, kobj, c, t))
    return keys[0], keys[1], rec, obj


@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_kernel_matches_the_restatement_on_adversarial_inputs(ctx, cam_kind):
    """Random and adversarial keys (NaN and inf colours, positions and depths, t = +inf, misses, huge colours that overflow the sums) under
    cameras that have translated and rotated so that taps straddle every image border, for every film size, at both keys' own times and
    between them, with the depth test tight, loose and at zero."""
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)  # hitables 1 (the fractal) and one sphere are animated: object motion is exercised too
    ctx.upload_world(wd)
    hit = T.world_hitables(wd)
    seen = set()
    for si, (w, h) in enumerate(SIZES + [(1, 1), (17, 13)]):
        for adversarial in (False, True):
            ka, kb, rec, obj = _random_case(w, h, 10 * si + adversarial, cam_kind, adversarial)
            for ts, tol in ((0.5, 0.05), (0.25, 0.0), (0.75, 1e30), (0.6, 0.25)):
                _, src = _check(ctx, w, h, ka, kb, rec, obj, ts, tol, hit, (w, h, adversarial, ts, tol))
                seen |= set(np.unique(src).tolist())
    assert seen == {0, 1, 2, 3, 4}


# ---- 3. rendered keys ---------------------------------------------------------------------------------------------------------------------

# (scene, camera, size): every scene, camera family and size occurs; the times below move camera and hitables far enough that the
# restatement, on the oracle's G-buffers, shows both keys, either key alone and the cross-fade (checked on the CPU before fixing them:
# s0 1338 / 103 / 95 / 0, s1 706 / 138 / 96 / 20, bulb 360 / 5 / 11 / 1474, multi 740 / 118 / 81 / 21 pixels of source 0 / 1 / 2 / 3).
RENDERED = [("s0", "pinhole", (48, 32)), ("s1", "thin", (40, 24)), ("bulb", "ortho", (50, 37)), ("multi", "pinhole", (40, 24))]
TIMES = (0.0, 0.25, 0.5)


@pytest.mark.parametrize("fma", [0, 1])
def test_kernel_on_rendered_keys_of_moving_scenes(ctx, fma):
    """Two rendered keys (GPU film, GPU G-buffer) and the frame between them of scenes whose camera, fractal and one sphere move: every
    plane and the source plane equal the restatement's, and over the set the sources 0, 1, 2 and 3 occur from the motion alone.  A finite
    film never takes source 4 - that needs a key pixel that is not finite - so on s1 one pixel of key A inside the cross-faded region is
    overwritten with an inf, as a firefly that overflowed would leave it: then every source 0..4 has occurred."""
    import rayn_amd as R
    ta, ts, tb = TIMES
    seen = set()
    for name, cam, (w, h) in RENDERED:
        wd, _, _ = scenes.scene(name, (w, h), cam, moving=True)
        ctx.set_fma_policy(fma)
        try:
            ps = [R.frame_params(w, h, 1, 2, frame=f, time_range=(t, t + 0.04)) for f, t in ((1, ta), (2, ts), (3, tb))]
            films = IO.render_frames(ctx, wd, [ps[0], ps[2]], 2)
            gb = [IO.gpu_gbuffer(ctx, p)[1:] for p in ps]
        finally:
            ctx.set_fma_policy(0)
        keys = [I.Key({k: v.cpu().numpy() for k, v in film.items()}, rec, obj, wd.camera, t) for film, (rec, obj), t in zip(films, (gb[0], gb[2]), (ta, tb))]
        hit = T.world_hitables(wd)
        _, src = _check(ctx, w, h, keys[0], keys[1], gb[1][0], gb[1][1], ts, 0.05, hit, (name, cam, fma))
        seen |= set(np.unique(src).tolist())
        if name == "s1":
            assert seen == {0, 1, 2, 3}  # s0 and s1 already show them
            q = int(np.flatnonzero(src == 3)[0])
            keys[0].film["color"].reshape(-1, 3)[q, 1] = np.inf
            _, src = _check(ctx, w, h, keys[0], keys[1], gb[1][0], gb[1][1], ts, 0.05, hit, (name, cam, fma, "firefly"))
            assert src[q] == 4
            seen |= set(np.unique(src).tolist())
    assert seen == {0, 1, 2, 3, 4}


# ---- 4. input hygiene ---------------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_invalid_arg_with_a_text(ctx):
    import torch
    import rayn_amd as R
    from rayn_amd import _abi
    L = ctx._L
    w, h = 40, 24
    n = w * h
    wd, _, _ = scenes.scene("s0", (w, h))
    fresh = R.Context(0)
    zeros = lambda k, dt=torch.float32: torch.zeros(k, dtype=dt, device="cuda")
    vp = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    cam = wd.camera
    bad_cam = _abi.Camera.from_buffer_copy(cam)
    bad_cam.kind = 9
    bufs = [{"color": zeros(3 * n), "alpha": zeros(n), "background": zeros(3 * n), "normal": zeros(3 * n), "rec": zeros(4 * n + 4), "obj": zeros(n + 1, torch.int32)}
            for _ in range(2)]
    grec, gobj = zeros(4 * n + 4), zeros(n + 1, torch.int32)
    outs = {"color": torch.full((3 * n,), 7.0, device="cuda"), "alpha": torch.full((n,), 7.0, device="cuda"), "background": torch.full((3 * n,), 7.0, device="cuda"),
            "normal": torch.full((3 * n,), 7.0, device="cuda"), "source": torch.full((n + 1,), -3, dtype=torch.int32, device="cuda")}

    def key(b, t, cam=cam, **kw):
        f = dict(d_color=vp(b["color"]), d_alpha=vp(b["alpha"]), d_background=vp(b["background"]), d_normal=vp(b["normal"]), d_records=vp(b["rec"]),
                 d_object=vp(b["obj"]), camera=None if cam is None else C.addressof(cam), time_start=t)
        f.update(kw)
        return _abi.InterpolateKey(**{k: (v.value if isinstance(v, C.c_void_p) else v) for k, v in f.items()})

    def call(c=ctx, p=R.frame_params(w, h, 1, 1, time_range=(0.5, 0.6)), ip=_abi.InterpolateParams(0.05), a="default", b="default", grec=vp(grec), gobj=vp(gobj),
             color=vp(outs["color"]), alpha=vp(outs["alpha"]), background=vp(outs["background"]), normal=vp(outs["normal"]), source=vp(outs["source"])):
        a = key(bufs[0], 0.0) if a == "default" else a
        b = key(bufs[1], 1.0) if b == "default" else b
        rc = L.rayn_hip_interpolate_device(c.h, None if p is None else C.byref(p), None if ip is None else C.byref(ip), None if a is None else C.byref(a),
                                           None if b is None else C.byref(b), grec, gobj, color, alpha, background, normal, source, None)
        return rc, c.last_error()

    try:
        assert call(c=fresh) == (-1, "rayn_hip_upload_world has not been called")
    finally:
        fresh.close()
    ctx.upload_world(wd)
    tp = lambda t: R.frame_params(w, h, 1, 1, time_range=(t, t + 0.1))
    nan, inf = float("nan"), float("inf")
    IP = _abi.InterpolateParams
    b0, b1 = bufs
    cases = [(dict(p=None), "null frame params"), (dict(ip=None), "null interpolate params"), (dict(a=None), "null key"), (dict(b=None), "null key"),
             (dict(p=R.frame_params(0, h, 1, 1)), "zero-sized"), (dict(p=R.frame_params(65536, 32768, 1, 1)), "2^31"),
             (dict(ip=IP(-0.1)), "depth_tolerance"), (dict(ip=IP(nan)), "depth_tolerance"), (dict(ip=IP(inf)), "depth_tolerance"),
             (dict(a=key(b0, 0.0, cam=None)), "null camera"), (dict(b=key(b1, 1.0, cam=bad_cam)), "unknown camera kind"),
             (dict(a=key(b0, nan)), "must be finite"), (dict(b=key(b1, inf)), "must be finite"), (dict(p=tp(nan)), "must be finite"),
             (dict(a=key(b0, 1.0)), "key A must lie before key B"), (dict(a=key(b0, 2.0)), "key A must lie before key B"),
             (dict(p=tp(-0.5)), "between the keys"), (dict(p=tp(1.5)), "between the keys"),
             (dict(a=key(b0, 0.0, d_color=None)), "null Color"), (dict(b=key(b1, 1.0, d_color=None)), "null Color"), (dict(color=None), "null Color"),
             (dict(a=key(b0, 0.0, d_records=None)), "null G-buffer"), (dict(b=key(b1, 1.0, d_object=None)), "null G-buffer"), (dict(grec=None), "null G-buffer"),
             (dict(gobj=None), "null G-buffer"),
             (dict(a=key(b0, 0.0, d_alpha=None)), "in both keys and the output"), (dict(b=key(b1, 1.0, d_background=None)), "in both keys and the output"),
             (dict(normal=None), "in both keys and the output"), (dict(a=key(b0, 0.0, d_normal=None), b=key(b1, 1.0, d_normal=None)), "in both keys and the output"),
             (dict(a=key(b0, 0.0, d_records=vp(b0["rec"], 4))), "16-byte aligned"), (dict(grec=vp(grec, 8)), "16-byte aligned"),
             (dict(b=key(b1, 1.0, d_object=vp(b1["obj"], 2))), "4-byte aligned"), (dict(gobj=vp(gobj, 1)), "4-byte aligned"), (dict(source=vp(outs["source"], 2)), "4-byte aligned"),
             (dict(color=vp(b0["color"])), "alias an input"), (dict(alpha=vp(b1["alpha"])), "alias an input"), (dict(background=vp(grec)), "alias an input"),
             (dict(source=vp(gobj)), "alias an input"), (dict(normal=vp(b1["rec"], 16)), "alias an input"),
             (dict(alpha=vp(outs["color"], 4)), "alias each other"), (dict(source=vp(outs["normal"])), "alias each other")]
    for kw, text in cases:
        rc, err = call(**kw)
        assert rc == -1 and text in err, (kw, rc, err)
    torch.cuda.synchronize()
    assert all(torch.all(outs[k] == 7.0) for k in ("color", "alpha", "background", "normal")) and torch.all(outs["source"] == -3), "a refused call wrote"
    # the valid call, ts at either key and with every optional plane absent
    assert call()[0] == 0 and call(p=tp(0.0))[0] == 0 and call(p=tp(1.0))[0] == 0
    none = dict(d_alpha=None, d_background=None, d_normal=None)
    assert call(a=key(b0, 0.0, **none), b=key(b1, 1.0, **none), alpha=None, background=None, normal=None, source=None)[0] == 0
    torch.cuda.synchronize()
    # Context.interpolate's own checks
    film = {"color": b0["color"]}
    g = {"records": b0["rec"], "object": b0["obj"]}
    p = tp(0.5)
    with pytest.raises(ValueError, match="_abi.Camera"):
        ctx.interpolate(p, R.Interpolate(), (film, g, None, 0.0), (film, g, cam, 1.0), g, {"color": outs["color"]})
    with pytest.raises(ValueError, match="color"):
        ctx.interpolate(p, R.Interpolate(), ({}, g, cam, 0.0), (film, g, cam, 1.0), g, {"color": outs["color"]})
    with pytest.raises(ValueError, match="d_out_source"):
        ctx.interpolate(p, R.Interpolate(), (film, g, cam, 0.0), (film, g, cam, 1.0), g, {"color": outs["color"]}, outs["color"])
    with pytest.raises(R.film.RaynHipError, match="alias"):
        ctx.interpolate(p, R.Interpolate(), (film, g, cam, 0.0), (film, g, cam, 1.0), g, {"color": b0["color"]})


# ---- 5. the sequence wiring and Film.interpolated -----------------------------------------------------------------------------------------

def _sequence_setup(w, h):
    import rayn_amd as R
    from rayn_amd import setup as S
    _, world, cam = scenes.scene("s1", (w, h), moving=True)
    integ = R.PathTracingIntegrator(max_bounces=2, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE)
    return world, cam, integ, R.BlackmanHarrisFilter(S.FILTER_RADIUS), S.TILE_SIZE


@pytest.mark.parametrize("every,frames,post", [(2, [2, 3, 4, 5, 6, 7], False), (3, [1, 2, 3, 4, 6, 7, 9], False), (2, [1, 2, 3, 4, 5], True)],
                         ids=["every2", "every3", "denoise-display"])
def test_render_sequence_with_interpolate_is_the_plain_keys_and_the_loop_of_the_entries(tmp_path, every, frames, post):
    """render_sequence(interpolate=Interpolate(k)): the images of the key frames are byte for byte those of the plain sequence, the images
    of every generated frame those of Context.gbuffer + Context.interpolate (+ denoise and display, whose auto-exposure state sees the
    frames in time order) on the same keys; the other channels' files likewise; the stats say which frames were generated."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    from rayn_amd import image
    K = R.ChannelKind
    w, h, samples = 48, 32, 1
    world, cam, integ, filt, tile = _sequence_setup(w, h)
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    itp = R.Interpolate(every, 0.05)
    dn = R.Denoise(2, 0.5, 0.4, 0.3) if post else None
    dp = R.Display(exposure="auto", adaptation=0.5, bloom=R.Bloom(levels=2)) if post else None
    film = R.Film(kinds, (w, h))
    stats = film.render_sequence(world, cam, integ, filt, tile, frames, 24, 1.0 / 24.0, samples, [K.Color, K.Alpha], str(tmp_path / "seq"), "a",
                                 denoise=dn, display=dp, interpolate=itp)
    got = IO.read_folder(tmp_path / "seq")
    suffix = "color_interp" + ("_denoised_display" if post else "")
    assert sorted(got) == sorted(f"a_{f:04d}_{s}.png" for f in frames for s in (suffix, "alpha"))
    is_key = [itp.is_key(i, len(frames)) for i in range(len(frames))]
    assert [s["frame"] for s in stats] == frames
    assert [bool(s.get("generated")) for s in stats] == [not k for k in is_key] and all(len(s) == 2 for s in stats if s.get("generated"))
    assert all("paths" in s for s, k in zip(stats, is_key) if k)
    if not post:  # (with a display the exposure state has seen other frames in between: the loop below covers the keys then)
        plain = R.Film(kinds, (w, h))
        keys = [f for f, k in zip(frames, is_key) if k]
        plain.render_sequence(world, cam, integ, filt, tile, keys, 24, 1.0 / 24.0, samples, [K.Color, K.Alpha], str(tmp_path / "plain"), "a")
        base = IO.read_folder(tmp_path / "plain")
        for f in keys:
            assert got[f"a_{f:04d}_color_interp.png"] == base[f"a_{f:04d}_color.png"], f
            assert got[f"a_{f:04d}_alpha.png"] == base[f"a_{f:04d}_alpha.png"], f
    # the loop of the entries
    ctx = film.ctx
    desc = world.to_desc(cam)
    ctx.upload_world(desc)
    mask = film.have_mask()

    def params(frame):
        start = f32(frame) * (f32(1.0) / f32(24))
        return start, R.frame_params(w, h, samples, 2, frame=frame, time_range=(float(start), float(f32(start + f32(1.0 / 24.0)))))

    rendered = {}
    for f, k in zip(frames, is_key):
        if k:
            _, p = params(f)
            out, g = F.alloc_device_film(w, h, "cuda"), F.alloc_gbuffer(w, h, "cuda")
            ctx.render_device(p, [torch.from_numpy(t).cuda() for t in R.build_tables(4 * samples, 2, p.volume_marches, f, w, h, filt)], out)
            ctx.gbuffer(p, g)
            rendered[f] = (out, g, p)
    state, shown_start = (ctx.display_state() if post else None), None
    img3, img1 = torch.empty(h * w * 3, dtype=torch.uint8, device="cuda"), torch.empty(h * w, dtype=torch.uint8, device="cuda")
    n_generated = 0
    for i, (f, k) in enumerate(zip(frames, is_key)):
        start, p = params(f)
        if k:
            d_film = rendered[f][0]
        else:
            fa = max(g for g, kk in zip(frames[:i], is_key[:i]) if kk)
            fb = min(g for g, kk in zip(frames[i + 1:], is_key[i + 1:]) if kk)
            g_t, d_film = F.alloc_gbuffer(w, h, "cuda"), F.alloc_device_film(w, h, "cuda")
            ctx.gbuffer(p, g_t)
            ctx.interpolate(p, itp, (rendered[fa][0], rendered[fa][1], desc.camera, rendered[fa][2].time_start),
                            (rendered[fb][0], rendered[fb][1], desc.camera, rendered[fb][2].time_start), g_t, d_film)
            n_generated += 1
        shown = d_film
        if post:
            den = torch.empty(w * h, 3, dtype=torch.float32, device="cuda")
            ctx.denoise(w, h, d_film, den, dn)
            shown = dict(d_film, color=den)
            ctx.display(dp, mask, False, w, h, shown, img3, state, None, 1.0 if shown_start is None else dp.adapt(float(start) - float(shown_start)))
            shown_start = start
        else:
            ctx.save_to_pixels(K.Color, mask, False, w, h, shown, img3)
        ctx.save_to_pixels(K.Alpha, mask, False, w, h, d_film, img1)
        image.save(str(tmp_path / "c.png"), img3.cpu().numpy().reshape(h, w, 3))
        image.save(str(tmp_path / "a.png"), img1.cpu().numpy().reshape(h, w, 1))
        assert open(tmp_path / "c.png", "rb").read() == got[f"a_{f:04d}_{suffix}.png"], (f, k)
        assert open(tmp_path / "a.png", "rb").read() == got[f"a_{f:04d}_alpha.png"], (f, k)
    assert n_generated == len(frames) - sum(is_key) >= 2
    # afterwards the film holds the last frame, a key
    assert torch.equal(film.channels["color"], rendered[frames[-1]][0]["color"])


def test_render_sequence_without_interpolate_is_unchanged_and_bad_orders_raise(tmp_path):
    import rayn_amd as R
    K = R.ChannelKind
    w, h = 40, 24
    world, cam, integ, filt, tile = _sequence_setup(w, h)
    kinds = [K.Color, K.Alpha, K.Background, K.WorldNormal]
    film = R.Film(kinds, (w, h))
    film.render_sequence(world, cam, integ, filt, tile, [1, 2], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "none"), "a", interpolate=None)
    one = R.Film(kinds, (w, h))
    for frame in (1, 2):
        one.render_frame_into(world, cam, integ, filt, tile, frame, IO.shutter_range(frame), 1)
        one.save_to([K.Color], str(tmp_path / "loop"), f"a_{frame:04d}")
    assert IO.read_folder(tmp_path / "none") == IO.read_folder(tmp_path / "loop")
    # one and two frames: nothing is generated
    st = film.render_sequence(world, cam, integ, filt, tile, [3], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "single"), "a", interpolate=R.Interpolate(4))
    assert sorted(IO.read_folder(tmp_path / "single")) == ["a_0003_color_interp.png"] and "generated" not in st[0]
    with pytest.raises((ValueError, R.film.RaynHipError)):
        film.render_sequence(world, cam, integ, filt, tile, [5, 4, 1], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "desc"), "a", interpolate=R.Interpolate(2))


def test_film_interpolated_equals_the_entry(tmp_path):
    """Film.interpolated(other, time_start): the planes of Context.gbuffer x 3 + Context.interpolate on the two films; the new film works
    with pixels, save_to, denoise=, display=, save_hdr and gbuffer(); the keys are not changed."""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    K = R.ChannelKind
    w, h = 50, 37
    world, cam, integ, filt, tile = _sequence_setup(w, h)
    kinds = [K.Color, K.Alpha, K.WorldNormal]
    fa, fb = R.Film(kinds, (w, h)), R.Film(kinds, (w, h))
    fa.render_frame_into(world, cam, integ, filt, tile, 1, (0.0, 0.04), 1)
    fb.render_frame_into(world, cam, integ, filt, tile, 2, (0.25, 0.29), 1)
    keep = {k: v.clone() for k, v in fa.channels.items()}
    itp = R.Interpolate(2, 0.1)
    gen = fa.interpolated(fb, 0.1, itp)
    assert gen.res == (w, h) and gen.channel_kinds == kinds and gen.ctx is fa.ctx and sorted(gen.channels) == ["alpha", "color", "normal"]
    ctx = fa.ctx
    pt = R.frame_params(w, h, 1, integ.max_bounces, frame=1, time_range=(float(f32(0.1)), 0.2))
    gs = [F.alloc_gbuffer(w, h, "cuda") for _ in range(3)]
    for p, g in zip((fa._last_params, fb._last_params, pt), gs):
        ctx.gbuffer(p, g)
    desc = world.to_desc(cam)
    want = {k: torch.empty_like(v) for k, v in gen.channels.items()}
    src = torch.empty(w * h, dtype=torch.int32, device="cuda")
    ctx.interpolate(pt, itp, ({k: fa.channels[k] for k in want}, gs[0], desc.camera, 0.0), ({k: fb.channels[k] for k in want}, gs[1], desc.camera, 0.25), gs[2], want, src)
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(gen.channels[k].view(torch.int32), want[k].view(torch.int32)), k
    assert len(torch.unique(src)) >= 3  # the frame is a real mixture
    assert all(torch.equal(fa.channels[k], keep[k]) for k in keep)
    g = gen.gbuffer()
    assert np.array_equal(g["object"].reshape(-1), gs[2]["object"].cpu().numpy().view(np.uint32))
    gen.save_to([K.Color, K.Alpha], str(tmp_path / "g"), "t", denoise=R.Denoise(1, 0.5, 0.4, 0.3), display=R.Display())
    gen.save_hdr(str(tmp_path / "g" / "t.pfm"), True)
    assert sorted(os.listdir(tmp_path / "g")) == ["t.pfm", "t_alpha.png", "t_color_denoised_display.png"]
    assert gen.pixels(K.WorldNormal).shape == (h, w, 3)
    for bad in (-0.1, 0.3, float("nan")):
        with pytest.raises(ValueError, match="between the keys"):
            fa.interpolated(fb, bad)
    with pytest.raises(ValueError, match="between the keys"):
        fb.interpolated(fa, 0.1)
    with pytest.raises(ValueError, match="no rendered frame"):
        fa.interpolated(R.Film(kinds, (w, h)), 0.1)
    with pytest.raises(ValueError, match="same size"):
        fa.interpolated(R.Film(kinds, (w, h + 1)), 0.1)


# ---- 6. does it do its job ----------------------------------------------------------------------------------------------------------------

# guided / cross-fade MSE ratios of the generated frames of tests/interpolate_np.InterpCase, computed with the CPU
# oracle and the numpy restatement (tools/interpolate_defaults.py --defaults) - the path the tests above hold the GPU to bit for bit.  Rows
# where the CPU run showed no gain over the cross-fade would not be asserted; there is none: at Interpolate()'s defaults the CPU run gave
# 0.5502, 0.5375, 0.4913, 0.4131 and 0.4509 for the five rows below.
QUALITY_ROWS = [(2, 2), (2, 4), (4, 2), (4, 3), (4, 4)]  # (every, generated frame)


def test_a_generated_frame_is_closer_to_the_truth_than_the_cross_fade():
    """InterpCase (the shipped scene at 160x96 under a fast camera drift, keys at samples=2): the MSE of the saturated Color + Background of
    every generated frame against a samples=256 render of that frame is below the plain cross-fade's of the same two keys.  Both are
    deterministic - the film is the oracle's bit for bit - so the comparison is direct; DESIGN.md section 8 cites the measured ratios."""
    import rayn_amd as R
    from rayn_amd import film as F
    D, IC = T.DefaultsCase, I.InterpCase
    wd, ps = IC.scene(D.SAMPLES)
    _, pref = IC.scene(D.REF_SAMPLES)
    c = R.Context(0)
    try:
        frames = IC.FRAMES
        noisy = dict(zip(frames, IO.render_frames(c, wd, [ps[f] for f in frames], D.BOUNCES)))
        want = {}
        for f, film in zip(frames[1:-1], IO.render_frames(c, wd, [pref[f] for f in frames[1:-1]], D.BOUNCES)):
            want[f] = np.clip(film["color"].cpu().numpy().astype(np.float64).reshape(D.H, D.W, 3) + film["background"].cpu().numpy().reshape(D.H, D.W, 3), 0.0, 1.0)
        gbuf = {}
        for f in frames:
            gbuf[f] = F.alloc_gbuffer(D.W, D.H, "cuda")
            c.gbuffer(ps[f], gbuf[f])
        itp = R.Interpolate()
        for every, f in QUALITY_ROWS:
            (_, fa, fb), = [r for r in IC.keys_of(every) if r[0] == f]
            out = F.alloc_device_film(D.W, D.H, "cuda")
            c.interpolate(ps[f], itp, (noisy[fa], gbuf[fa], wd.camera, ps[fa].time_start), (noisy[fb], gbuf[fb], wd.camera, ps[fb].time_start), gbuf[f], out)
            host = lambda film: {k: film[k].cpu().numpy() for k in ("color", "background")}
            x = IC.cross_fade(host(noisy[fa]), host(noisy[fb]), ps[fa].time_start, ps[fb].time_start, ps[f].time_start)
            guided, fade = D.mse(out["color"].cpu().numpy(), out["background"].cpu().numpy(), want[f]), D.mse(x["color"], x["background"], want[f])
            print(f"every {every} frame {f}: guided {guided:.6f} cross-fade {fade:.6f} ratio {guided / fade:.4f}")
            assert guided < fade, (every, f, guided, fade)
    finally:
        c.close()
