"""Inputs shared by tests/test_temporal_resample.py (CPU) and tests/test_temporal_resample_device.py (GPU): adversarial frames and histories
in the manner of temporal_cases.random_inputs, but with object REGIONS instead of per-pixel random objects, a sub-two-pixel
reprojection and a defect density low enough that whole 4x4 footprints survive - so that the restatement sends a sizeable share of the
pixels down each of the three arms (reset, bilinear fallback, Catmull-Rom).  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import scenes
import temporal_np as T

f32 = np.float32
W, H = 37, 29  # no multiple of 16, three blocks each way
MIN_SHARE = {2: 0.25, 1: 0.15, 0: 0.05}  # arm code -> the least share of the pixels that must take it
PREV_TIME, CUR_TIME = 0.25, 0.75


def adversarial_inputs(seed, cam_kind, w=W, h=H):
    """(prev_cam, color, normal, rec, obj, (A, B, N, O), moments (n, 2)) around the plane z = 0: three object bands with seams and a block of
    misses, a previous camera 1.3 / 0.6 pixels aside (rotated and animated too for the perspective kinds), and, on a few per cent of the
    pixels each, n = 0 taps, depth outliers, flipped normals, wrong objects, NaN / inf / huge values in every plane."""
    from rayn_amd import _abi
    rng = np.random.default_rng(seed)
    n = w * h
    pixel = 4.0 / h
    prev_cam = T.ortho_camera(w, h, origin_x=1.3 * pixel, pixel=pixel)
    prev_cam.origin.y = prev_cam.at.y = -0.6 * pixel
    if cam_kind != _abi.CAM_ORTHOGRAPHIC:
        prev_cam.kind, prev_cam.vfov_or_size = cam_kind, 53.0
        prev_cam.at.x += 0.02  # a rotation as well
        prev_cam.animated, prev_cam.origin_vel.z, prev_cam.up_vel.x = 1 | 4, 0.05, 0.02
    rec, _, normal = T.ortho_plane_gbuffer(w, h, pixel=pixel)
    rec[:, 2] = rng.normal(0.0, 0.02, n)
    xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    bands = np.where(xs < w // 3, 0, np.where(xs < 2 * w // 3, 1, 2)).astype(np.uint32)
    bands[(ys >= h - 6) & (xs >= w - 9)] = 0xFFFFFFFF
    obj = bands.reshape(-1).copy()
    obj[rng.random(n) < 0.03] = 0xFFFFFFFF
    rec[obj == T.MISS] = (0.0, 0.0, 0.0, np.inf)
    normal = (normal + rng.normal(0.0, 0.05, (n, 3))).astype(f32)
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(f32)
    ok, _, _, te = T.project(prev_cam, PREV_TIME, [rec[:, 0], rec[:, 1], rec[:, 2]], w, h)
    depth = float(np.nanmedian(te[ok & np.isfinite(te)]))
    lengths = rng.choice(np.array([1.0, 2.0, 3.5, 8.0]), n)
    lengths[rng.random(n) < 0.003] = 0.0
    A = np.concatenate([rng.gamma(0.6, 0.5, (n, 3)), lengths[:, None]], axis=1).astype(f32)
    tdepth = np.where(ok & np.isfinite(te), te, depth) * (1.0 + rng.normal(0.0, 0.004, n))  # about what the projection will expect
    tdepth[rng.random(n) < 0.003] *= 1.2
    B = np.concatenate([rng.normal(size=(n, 3)), tdepth[:, None]], axis=1).astype(f32)
    N = np.concatenate([np.tile([0.0, 0.0, 1.0], (n, 1)) + rng.normal(0.0, 0.05, (n, 3)), np.zeros((n, 1))], axis=1).astype(f32)
    N[rng.random(n) < 0.003, :3] *= f32(-1.0)
    O = bands.reshape(-1).copy()
    O[rng.random(n) < 0.003] = 7
    M = np.stack([rng.gamma(0.6, 0.5, n), rng.gamma(0.6, 0.8, n)], axis=1).astype(f32)
    special = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 3.0e38, -3.0e38, 1e-45, 1e30, -1e30], f32)
    for k, plane in enumerate((color, normal, rec, A, B, N, M)):  # four per plane: every one of them costs up to 16 pixels their footprint
        flat = plane.reshape(-1)
        idx = rng.choice(flat.size, 4, replace=False)
        flat[idx] = np.roll(special, -3 * k)[:4]
    return prev_cam, color, normal, rec, obj, (A, B, N, O), M


def moving_world(res=(40, 24)):
    """(world description, its hitables as temporal_np.accumulate takes them): scenes.scene's moving s1 - the fractal (object 1)
    and one sphere are animated - with the velocities cut to a tenth, so that over the half second between the two frames object motion
    shifts the footprints by a fraction of a pixel instead of tearing them apart."""
    wd, _, _ = scenes.scene("s1", res, moving=True)
    for i in range(wd.n_hitables):
        for c in "xyz":
            setattr(wd.hitables[i].center_vel, c, 0.1 * getattr(wd.hitables[i].center_vel, c))
    return wd, T.world_hitables(wd)


def non_finite_history_case(w=12, h=10, sx=0.5, sy=0.25):
    """(prev_cam, color, normal, rec, obj, prev, moments, clean A, clean moments) of the exact orthographic case - every tap valid, the
    previous camera sx / sy pixels aside - with non-finite history colours and moments placed where whole footprints contain them,
    independent of any seed's luck.  The weights of the inner taps are positive and those of the outer ring are not, so:
      a single +inf: the 12 footprints that hold it as an outer tap sum to -inf, and the clamp brings that back to the inner minimum; the 4
        that hold it as an inner tap sum to +inf, the inner maximum is +inf too, h stays +inf, the blend is NaN and step 5 resets the pixel;
      a single NaN: all 16 footprints sum to NaN and the clamp, whose fmaxf / fminf drop a NaN, returns the finite inner bound;
      a 2x2 block of +inf: a footprint that has block pixels both inside and on its ring sums to NaN and is healed like that; the one
        whose four inner taps are the block resets;
      a +inf first moment: the moments fall back to (y, y2) or are healed by the clamp while the colour keeps its blend."""
    rng = np.random.default_rng(21)
    n = w * h
    rec, obj, normal = T.ortho_plane_gbuffer(w, h)
    prev_cam = T.ortho_camera(w, h, origin_x=-sx * 0.125)
    prev_cam.origin.y = prev_cam.at.y = -sy * 0.125
    prev_rec, _, _ = T.ortho_plane_gbuffer(w, h, origin_x=-sx * 0.125)
    prev_rec[:, 1] -= f32(sy * 0.125)
    clean_A = np.concatenate([rng.random((n, 3)), rng.choice(np.array([1.0, 2.0, 5.0]), n)[:, None]], axis=1).astype(f32)
    clean_M = rng.random((n, 2)).astype(f32)
    A, M = clean_A.copy(), clean_M.copy()
    A[3 + 2 * w, 0] = np.inf
    A[3 + 6 * w, 2] = np.nan
    for x, y in ((8, 5), (9, 5), (8, 6), (9, 6)):
        A[x + y * w, 1] = np.inf
    M[6 + 3 * w, 0] = np.inf
    N = np.concatenate([normal, np.zeros((n, 1), f32)], axis=1)
    return prev_cam, rng.random((n, 3)).astype(f32), normal, rec, obj, (A, prev_rec, N, obj), M, clean_A, clean_M


def arm_shares(arm):
    return {code: float((np.asarray(arm) == code).mean()) for code in (0, 1, 2)}
