"""Inputs shared by the temporal tests - tests/test_temporal_device.py, test_temporal_variance_device.py, test_temporal_resample_device.py,
test_interpolate_device.py (GPU) and test_temporal_feedback.py (CPU) - and the accumulate entries' wrapper on host arrays.
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import device_io as IO
import temporal_np as T

f32 = np.float32
SIZES = [(48, 32), (40, 24), (50, 37)]  # whole 16x16 blocks; a width that is no multiple of 16; a size rayn's tile grid under-covers
SPECIAL = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, 1e30, -1e30], f32)
GUARD = 64


def random_inputs(w, h, seed, cam_kind, adversarial):
    """A current frame and a previous history around the plane z = 0 seen by two different cameras, with random objects, depths near the
    true ones, normals near +z and history lengths 0..cap; `adversarial` scatters NaN / inf / huge values over every plane."""
    from rayn_amd import _abi
    rng = np.random.default_rng(seed)
    n = w * h
    cur = T.ortho_camera(w, h, pixel=4.0 / h)
    prev_cam = T.ortho_camera(w, h, origin_x=float(rng.uniform(-0.6, 0.6)), pixel=4.0 / h)
    prev_cam.origin.y = prev_cam.at.y = float(rng.uniform(-0.5, 0.5))
    if cam_kind != _abi.CAM_ORTHOGRAPHIC:
        for c in (cur, prev_cam):
            c.kind, c.vfov_or_size = cam_kind, 53.0
        prev_cam.at.x += 0.3  # a rotation as well
        prev_cam.animated, prev_cam.origin_vel.z, prev_cam.up_vel.x = 1 | 4, 0.5, 0.2
    # current G-buffer: the plane's points under the current pixel centres (any camera kind may be handed any positions)
    rec, obj, normal = T.ortho_plane_gbuffer(w, h, pixel=4.0 / h)
    rec[:, 2] = rng.normal(0.0, 0.05, n)
    obj = rng.choice(np.array([0, 1, 1, 1, 2, 0xFFFFFFFF], np.uint32), n)
    rec[obj == T.MISS] = (0.0, 0.0, 0.0, np.inf)
    normal = (normal + rng.normal(0.0, 0.3, (n, 3))).astype(f32)
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
    # previous history: depths scattered around what the projection will expect (4 for the orthographic camera), lengths 0 .. 8
    ok, fx, fy, te = T.project(prev_cam, 0.25, [rec[:, 0], rec[:, 1], rec[:, 2]], w, h)
    A = np.concatenate([rng.gamma(0.6, 0.5, (n, 3)), rng.choice(np.array([0.0, 1.0, 2.0, 3.5, 8.0]), n)[:, None]], axis=1).astype(f32)
    B = np.concatenate([rng.normal(size=(n, 3)), (np.nanmedian(te[ok]) if ok.any() else 4.0) * rng.choice(np.array([1.0, 1.0, 1.02, 0.97, 1.2]), n)[:, None]], axis=1).astype(f32)
    N = np.concatenate([np.tile([0.0, 0.0, 1.0], (n, 1)) + rng.normal(0.0, 0.3, (n, 3)), np.zeros((n, 1))], axis=1).astype(f32)
    O = rng.choice(np.array([0, 1, 1, 1, 2, 0xFFFFFFFF], np.uint32), n)
    if adversarial:
        for plane in (color, normal, rec, A, B, N):
            flat = plane.reshape(-1)
            idx = rng.choice(flat.size, min(flat.size // 4, 6 * SPECIAL.size), replace=False)
            flat[idx] = np.resize(SPECIAL, idx.size)
    return cur, prev_cam, color, normal, rec, obj, (A, B, N, O)


# the Temporal parameter sets of tests/test_temporal_device.py::test_accumulate_matches_the_restatement_on_adversarial_inputs
ADVERSARIAL_PARAMS = [(4, 0.05, -1.0), (1, 0.05, 0.9), (8, 0.0, 0.5), (3, 1e30, 1.0), (65536, 0.25, -1.0)]
INTEGRAL_SHIFTS = ((0.0, 0.0), (3.0, 0.0), (-2.25, 0.0), (0.0, 2.0), (0.5, -1.75), (-20.0, 0.0))


def older_accumulate_calls():
    """The arguments of every temporal_np.accumulate call whose result tests/test_temporal_device.py compares the kernel with in
    test_accumulate_matches_the_restatement_on_adversarial_inputs and test_accumulate_on_exactly_integral_reprojections (111 calls; the
    calls without a history aside).  A COPY of those two tests' loops, for tests/test_reproject_cases.py to measure what their inputs can
    see: whoever changes the loops there changes them here (both tests carry a note), and the count asserted there guards the copy."""
    import scenes
    wd, _, _ = scenes.scene("s1", (40, 24), moving=True)
    hit = T.world_hitables(wd)
    for cam_kind in (0, 1, 2):
        for si, (w, h) in enumerate(SIZES + [(1, 1), (17, 13)]):
            for adversarial in (False, True):
                cur, prev_cam, color, normal, rec, obj, prev = random_inputs(w, h, 10 * si + adversarial, cam_kind, adversarial)
                for tp in ADVERSARIAL_PARAMS[(si + adversarial) % 2::2] if w > 17 else ADVERSARIAL_PARAMS:
                    yield (w, h, color, normal, rec, obj, prev, prev_cam, 0.25, 0.75, hit, *tp)
    w, h = 16, 8
    rec, obj, normal = T.ortho_plane_gbuffer(w, h)
    rng = np.random.default_rng(3)
    for sx, sy in INTEGRAL_SHIFTS:
        prev_cam = T.ortho_camera(w, h, origin_x=-sx * 0.125)
        prev_cam.origin.y = prev_cam.at.y = -sy * 0.125
        prev_rec, _, _ = T.ortho_plane_gbuffer(w, h, origin_x=-sx * 0.125)
        prev_rec[:, 1] -= f32(sy * 0.125)
        A = np.concatenate([rng.random((w * h, 3)), np.full((w * h, 1), 3.0)], axis=1).astype(f32)
        prev = (A, prev_rec, np.concatenate([normal, np.zeros((w * h, 1), f32)], axis=1), obj)
        color = rng.random((w * h, 3)).astype(f32)
        yield (w, h, color, normal, rec, obj, prev, prev_cam, 0.0, 0.0, [], 3, 0.05, 0.9)


def pack_inputs(w, h, seed):
    """Synthetic inputs of the denoise entry: a patchwork of objects with misses, history lengths 0, 1, 3, 3.5, 4, 8 and NaN side by side,
    special values over colour, guides and moments."""
    rng = np.random.default_rng(seed)
    n = w * h
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
    normal = rng.normal(size=(n, 3)).astype(f32)
    alpha = rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 1.0], f32), n)
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    patch = rng.choice(np.array([0, 1, 1, 2, 0xFFFFFFFF], np.uint32), (h // 4 + 1, w // 5 + 1))
    obj = patch[ys // 4, xs // 5].reshape(-1).copy()
    obj[rng.choice(n, n // 20, replace=False)] = 3  # single pixels of another object inside the patches
    n1 = rng.choice(np.array([0.0, 1.0, 1.0, 3.0, 3.5, 4.0, 8.0], f32), n)
    if n >= 4:
        n1[rng.choice(n, 4, replace=False)] = (np.nan, np.inf, -1.0, 0.5)
    m1 = rng.gamma(0.6, 0.5, n).astype(f32)
    mom = np.stack([m1, (m1 * m1 + rng.normal(0.0, 0.05, n)).astype(f32)], axis=1).astype(f32)  # m2 - m1^2 of either sign
    for arr in (color, normal, alpha, mom):
        flat = arr.reshape(-1)
        idx = rng.choice(flat.size, min(flat.size, 3 * SPECIAL.size), replace=False)
        flat[idx] = np.resize(SPECIAL, idx.size)
    A = np.concatenate([rng.random((n, 3)).astype(f32), n1[:, None]], axis=1).astype(f32)  # the entry reads only n' of the history
    hist = T.join_history(A, rng.random((n, 4)).astype(f32), rng.random((n, 4)).astype(f32), obj)
    return {"color": color, "normal": normal, "alpha": alpha, "obj": obj, "n1": n1, "mom": mom, "hist": hist}


def gpu_accumulate(ctx, p, temporal, color, normal, rec, obj, prev, prev_mom, prev_cam, prev_time, moments=True, entry=None):
    """An accumulate entry on host arrays: (out (n, 3), (A, B, N, O), moments (n, 2) or None).  Context.temporal_accumulate, or `entry`
    (film, g, d_prev, d_new, d_out, d_prev_moments, d_new_moments or None), which makes the call itself.  Checks the guard bytes behind
    every output - the whole moments buffer when it is not handed over - and that the previous buffers and the inputs were left alone."""
    import torch
    from rayn_amd import film as F
    n = p.width * p.height
    film = {"color": IO.upload(color), "normal": IO.upload(normal)}
    g = IO.upload_gbuffer(rec, obj)
    d_prev = None if prev is None else IO.upload_bytes(T.join_history(*prev))
    d_pm = None if prev is None or prev_mom is None or not moments else IO.upload_bytes(np.asarray(prev_mom, f32))
    keep = IO.snapshot([d_prev, d_pm])
    hb, mb = F.temporal_history_bytes(p.width, p.height), F.temporal_moments_bytes(p.width, p.height)
    full_new, d_new = IO.guarded(hb, torch.uint8, 0xA5, GUARD)
    full_nm, d_nm = IO.guarded(mb, torch.uint8, 0xA5, GUARD)
    full_out, d_out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
    if entry is None:
        ctx.temporal_accumulate(p, temporal, film, g, d_prev, prev_cam, prev_time, d_new, d_out, None, d_pm, d_nm if moments else None)
    else:
        entry(film, g, d_prev, d_new, d_out, d_pm, d_nm if moments else None)
    torch.cuda.synchronize()
    IO.assert_guards(full_new, hb, 0xA5, "new history")
    IO.assert_guards(full_out, 3 * n, 7.0, "colour")
    IO.assert_guards(full_nm, mb if moments else 0, 0xA5, "new moments")
    IO.assert_unchanged([d_prev, d_pm], keep, "a previous buffer")
    IO.assert_is_host(film["color"], color, "color")
    IO.assert_is_host(film["normal"], normal, "normal")
    IO.assert_gbuffer_is_host(g, rec, obj, "G-buffer")
    mom = d_nm.cpu().numpy().view(f32).reshape(n, 2) if moments else None
    return d_out.cpu().numpy().reshape(n, 3), T.split_history(d_new.cpu().numpy(), n), mom


def assert_history_equal(got, want, what):
    """The planes A, B and N of two histories bit for bit (NaN payloads aside), the objects equal"""
    for name, a, b in zip("ABN", got[:3], want[:3]):
        IO.assert_bits_equal(a, b, (what, name))
    assert np.array_equal(got[3], want[3]), (what, "object")


def defaults_case_errors(tp, dn=None, moments=True, feedback=False):
    """temporal_np.DefaultsCase (shipped scene, 160x96, moving camera, 8 frames, against samples=256) on a context of its own: the frames
    accumulated under the Temporal `tp` (through the moments entry unless moments=False) and filtered by the VarianceDenoise `dn` - after
    the last frame or, with `feedback`, after every frame with tp.feedback, each feeding the next frame's history.
    -> the MSEs of (the raw last frame, the accumulated one, the filtered one or None)"""
    import torch
    import rayn_amd as R
    from rayn_amd import film as F
    D = T.DefaultsCase
    wd, ps, pref = D.scene()
    c = R.Context(0)
    try:
        frames = IO.render_frames(c, wd, ps + [pref], D.BOUNCES)
        ref = frames.pop()
        want = np.clip(ref["color"].cpu().numpy().reshape(D.H, D.W, 3).astype(np.float64) + ref["background"].cpu().numpy().reshape(D.H, D.W, 3), 0.0, 1.0)
        hist = [torch.empty(F.temporal_history_bytes(D.W, D.H), dtype=torch.uint8, device="cuda") for _ in range(2)]
        mom = [torch.empty(F.temporal_moments_bytes(D.W, D.H), dtype=torch.uint8, device="cuda") for _ in range(2)] if moments else None
        g, acc = F.alloc_gbuffer(D.W, D.H, "cuda"), torch.empty(D.W * D.H, 3, dtype=torch.float32, device="cuda")
        shown = None if dn is None else torch.empty_like(acc)
        for i, (p, film) in enumerate(zip(ps, frames)):
            c.gbuffer(p, g)
            with_moments = (None, None if i == 0 else mom[(i + 1) % 2], mom[i % 2]) if moments else ()
            c.temporal_accumulate(p, tp, film, g, None if i == 0 else hist[(i + 1) % 2], None if i == 0 else wd.camera,
                                  0.0 if i == 0 else ps[i - 1].time_start, hist[i % 2], acc, *with_moments)
            if feedback:
                c.denoise_temporal_variance(D.W, D.H, dict(film, color=acc), g, hist[i % 2], mom[i % 2], shown, dn, feedback=tp.feedback)
        last, k = frames[-1], (len(ps) - 1) % 2
        if dn is not None and not feedback:
            c.denoise_temporal_variance(D.W, D.H, dict(last, color=acc), g, hist[k], mom[k], shown, dn)
        torch.cuda.synchronize()
        bg = last["background"].cpu().numpy().reshape(D.H, D.W, 3)
        return tuple(None if x is None else D.mse(x.cpu().numpy(), bg, want) for x in (last["color"], acc, shown))
    finally:
        c.close()
