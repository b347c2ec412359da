"""numpy restatement of the temporal accumulation (rayn_hip_temporal_accumulate_device; the definition is in include/rayn_hip.h) and of
the G-buffer's assembly P = o + t * d, binary32 operation by operation with the f32 helpers of tests/restatement_np.py.  It shares no code
with rayn_amd/csrc/temporal.hip; tests/test_temporal_device.py compares the two bit for bit.  TEST INFRASTRUCTURE: nothing under rayn_amd/
imports this.

MUTANTS names the wrong readings of one decision each that the cases of tests/reproject_cases.py have to tell from the statement
(project(..., mutant=) and accumulate(..., mutant=); mutant=None is the statement).  EQUIVALENT names two readings that look wrong and
are not - no input tells them from the statement, so they are accepted by the functions (tests/test_reproject_cases.py holds every case
to it) and kept out of MUTANTS:
  zc_ge  perspective `zc > 0` read as `zc >= 0`.  zc = +-0 makes the divisor zc * half_w a zero, so uvx is +-inf or (0 / 0) NaN, and so
         is fx = uvx * width - 0.5: the projection is rejected by its finiteness test whatever the sign test said.
  w_ge   `W > 0` read as `W >= 0`.  The bilinear weights are >= 0, so W = 0 means every tap that counted had weight 0: S = 0 (or NaN),
         h = S / W = 0 / 0 is NaN, the blend is not finite and the pixel resets exactly as it does for W <= 0."""
import math

import numpy as np

from restatement_np import PI, f32, vscale, vsub

MISS = np.uint32(0xFFFFFFFF)
MUTANTS = ("depth_lt",             # |t_tap - te| < tol
           "normal_gt",            # dot(nrm, nrm_tap) > normal_min
           "ntap_gt",              # n_tap > 1
           "normal_switch_ge",     # the normal test stays on at normal_min == -1
           "te_ge",                # orthographic: a point on the camera plane is accepted (te >= 0)
           "fmin_is_minimum",      # n' = min(nh + 1, max_history) with a NaN nh propagating
           "cap_after_add",        # n' = fmin(nh, max_history) + 1
           "tap_inside_le",        # a tap counts as inside up to qx == width and qy == height (read from the clamped pixel)
           "zero_weight_skipped",  # a tap of weight 0 does not count (k_interpolate's and k_upscale's rule)
           "reset_keeps_length")   # n' = 1 for a colour that is not finite
EQUIVALENT = ("zc_ge", "w_ge")


def _known(mutant):
    assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant


# ---- the definition's own vector forms (NOT rayn's: no mul_add, a plain left-to-right dot) ------------------------------------------------
def dot(a, b):
    return ((a[0] * b[0]).astype(f32) + (a[1] * b[1]).astype(f32)).astype(f32) + (a[2] * b[2]).astype(f32)


def cross(a, b):
    return [((a[1] * b[2]).astype(f32) - (a[2] * b[1]).astype(f32)).astype(f32), ((a[2] * b[0]).astype(f32) - (a[0] * b[2]).astype(f32)).astype(f32),
            ((a[0] * b[1]).astype(f32) - (a[1] * b[0]).astype(f32)).astype(f32)]


def nz(a):
    with np.errstate(all="ignore"):
        r = (f32(1.0) / np.sqrt(dot(a, a)).astype(f32)).astype(f32)
    return vscale(a, r)


def _v(v):
    return [np.asarray(f32(v.x)), np.asarray(f32(v.y)), np.asarray(f32(v.z))]


def camera_constants(cam):
    """(half_w, half_h, full_w, full_h) as the cameras' ::new derive them (src/camera.rs:53-72,134-157,228-240)"""
    res_w, res_h = f32(cam.res_w), f32(cam.res_h)
    if cam.kind in (0, 1):
        theta = f32(f32(f32(cam.vfov_or_size) * PI) / f32(180.0))
        half_h = f32(math.tan(float(f32(theta / f32(2.0)))))
        half_w = f32(f32(res_w / res_h) * half_h)
        return half_w, half_h, half_w, half_h
    vsz = f32(cam.vfov_or_size)
    full_w, full_h = f32(vsz * f32(res_w / res_h)), vsz
    return f32(full_w / f32(2.0)), f32(full_h / f32(2.0)), full_w, full_h


def gbuffer_assemble(org, dirs, t, obj):
    """The G-buffer records (n, 4) and objects from the pixel-centre rays and the closest hits: P = o + t * d as a multiply and an add; a
    miss is (0, 0, 0, +inf) and 0xFFFFFFFF."""
    org, dirs = np.asarray(org, f32).reshape(-1, 3), np.asarray(dirs, f32).reshape(-1, 3)
    t, obj = np.asarray(t, f32).reshape(-1), np.asarray(obj, np.uint32).reshape(-1)
    with np.errstate(all="ignore"):
        P = (org + (t[:, None] * dirs).astype(f32)).astype(f32)
    rec = np.concatenate([P, t[:, None]], axis=1).astype(f32)
    miss = obj == MISS
    rec[miss] = np.array([0.0, 0.0, 0.0, np.inf], f32)
    return rec, obj.copy()


def split_history(hist, n):
    """(A (n, 4), B (n, 4), normal (n, 4), object (n,)) views of one history block (52 bytes per pixel)"""
    b = np.asarray(hist).view(np.uint8).reshape(-1)
    return (b[: 16 * n].view(f32).reshape(n, 4), b[16 * n: 32 * n].view(f32).reshape(n, 4), b[32 * n: 48 * n].view(f32).reshape(n, 4),
            b[48 * n: 52 * n].view(np.uint32))


def join_history(A, B, N, O):
    return np.concatenate([np.ascontiguousarray(A, f32).reshape(-1).view(np.uint8), np.ascontiguousarray(B, f32).reshape(-1).view(np.uint8),
                           np.ascontiguousarray(N, f32).reshape(-1).view(np.uint8), np.ascontiguousarray(O, np.uint32).reshape(-1).view(np.uint8)])


def project(cam, ts_prev, Pp, width, height, mutant=None):
    """Step 3 for the points Pp (three arrays): (ok, fx, fy, te)."""
    _known(mutant)
    half_w, half_h, full_w, full_h = camera_constants(cam)
    ts = f32(ts_prev)

    def closure(base, vel, bit):
        b = _v(base)
        if not (cam.animated & bit):
            return b
        vv = _v(vel)
        return [(b[c] + (vv[c] * ts).astype(f32)).astype(f32) for c in range(3)]

    o, at, up = closure(cam.origin, cam.origin_vel, 1), closure(cam.at, cam.at_vel, 2), closure(cam.up, cam.up_vel, 4)
    with np.errstate(all="ignore"):
        if cam.kind == 2:
            w = nz(vsub(at, o))
            u = nz(cross(w, up))
            v = cross(u, w)
            ll = vsub(vsub(o, vscale(u, half_w)), vscale(v, half_h))
            q = vsub(Pp, ll)
            uvx = (dot(q, u) / full_w).astype(f32)
            uvy = (dot(q, v) / full_h).astype(f32)
            te = dot(q, w).astype(f32)
            ok = te >= 0 if mutant == "te_ge" else te > 0
        else:
            w = nz(vsub(o, at))
            u = nz(cross(up, w))
            v = cross(w, u)
            q = vsub(Pp, o)
            zc = (-dot(q, w)).astype(f32)
            ok = zc >= 0 if mutant == "zc_ge" else zc > 0
            uvx = (((dot(q, u) / (zc * half_w).astype(f32)).astype(f32) + f32(1.0)).astype(f32) * f32(0.5)).astype(f32)
            uvy = (((dot(q, v) / (zc * half_h).astype(f32)).astype(f32) + f32(1.0)).astype(f32) * f32(0.5)).astype(f32)
            te = np.sqrt(dot(q, q)).astype(f32)
        fx = ((uvx * f32(width)).astype(f32) - f32(0.5)).astype(f32)
        fy = ((uvy * f32(height)).astype(f32) - f32(0.5)).astype(f32)
    ok = ok & np.isfinite(fx) & np.isfinite(fy)
    return ok, fx, fy, te


def accumulate(width, height, color, normal, rec, obj, prev, prev_cam, prev_time, cur_time, hitables, max_history, depth_tolerance, normal_min,
               want_taps=False, mutant=None):
    """One temporal accumulate.  color / normal (n, 3), rec (n, 4), obj (n,) of the current frame; prev = the previous history as
    (A, B, N, O) or None; hitables = [(animated, (vx, vy, vz))] of the world.  Returns (out colour (n, 3), (A', B', N', O')) and, with
    want_taps, also the per-pixel summed tap weight W (0 where the pixel reset before its taps)."""
    _known(mutant)
    n = width * height
    color, normal = np.asarray(color, f32).reshape(n, 3), np.asarray(normal, f32).reshape(n, 3)
    rec, obj = np.asarray(rec, f32).reshape(n, 4), np.asarray(obj, np.uint32).reshape(n)
    cfin = np.isfinite(color).all(axis=1)
    out = color.copy()
    nn = np.where(cfin, f32(1.0), f32(1.0 if mutant == "reset_keeps_length" else 0.0)).astype(f32)
    Wsum = np.zeros(n, f32)
    go = cfin & (obj != MISS)
    if prev is not None and go.any():
        pA, pB, pN, pO = [np.asarray(a) for a in prev]
        pA, pB, pN, pO = pA.reshape(n, 4), pB.reshape(n, 4), pN.reshape(n, 4), pO.reshape(n)
        with np.errstate(all="ignore"):
            dt = f32(f32(cur_time) - f32(prev_time))
            Pp = [rec[:, c].copy() for c in range(3)]
            for k, (animated, vel) in enumerate(hitables):
                if animated:
                    m = obj == k
                    for c in range(3):
                        Pp[c] = np.where(m, (rec[:, c] - (f32(vel[c]) * dt).astype(f32)).astype(f32), Pp[c]).astype(f32)
            ok, fx, fy, te = project(prev_cam, prev_time, Pp, width, height, mutant)
            ok = ok & go
            x0f, y0f = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
            wx1, wy1 = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
            wx0, wy0 = (f32(1.0) - wx1).astype(f32), (f32(1.0) - wy1).astype(f32)
            x0 = np.clip(np.where(np.isfinite(x0f), x0f, f32(-2.0)), f32(-2.0), f32(2147483648.0)).astype(np.int64)
            y0 = np.clip(np.where(np.isfinite(y0f), y0f, f32(-2.0)), f32(-2.0), f32(2147483648.0)).astype(np.int64)
            tol = (f32(depth_tolerance) * te).astype(f32)
            W, S, N = np.zeros(n, f32), np.zeros((n, 3), f32), np.zeros(n, f32)
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                inside = ok & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                q = np.where(inside, qx + qy * width, 0)
                if mutant == "tap_inside_le":
                    inside = ok & (qx >= 0) & (qx <= width) & (qy >= 0) & (qy <= height)
                    q = np.where(inside, np.minimum(qx, width - 1) + np.minimum(qy, height - 1) * width, 0)
                a = pA[q]
                dd = np.abs((pB[q, 3] - te).astype(f32))
                use = inside & (a[:, 3] > f32(1.0) if mutant == "ntap_gt" else a[:, 3] >= f32(1.0)) & (pO[q] == obj)
                use &= dd < tol if mutant == "depth_lt" else dd <= tol
                if f32(normal_min) >= f32(-1.0) if mutant == "normal_switch_ge" else f32(normal_min) > f32(-1.0):
                    nq = pN[q]
                    dn = dot([normal[:, 0], normal[:, 1], normal[:, 2]], [nq[:, 0], nq[:, 1], nq[:, 2]])
                    use &= dn > f32(normal_min) if mutant == "normal_gt" else dn >= f32(normal_min)
                w = ((wx1 if k & 1 else wx0) * (wy1 if k >> 1 else wy0)).astype(f32)
                if mutant == "zero_weight_skipped":
                    use &= w > 0
                W = np.where(use, (W + w).astype(f32), W).astype(f32)
                for c in range(3):
                    S[:, c] = np.where(use, (S[:, c] + (w * a[:, c]).astype(f32)).astype(f32), S[:, c])
                N = np.where(use, (N + (w * a[:, 3]).astype(f32)).astype(f32), N).astype(f32)
            have = ok & (W >= 0 if mutant == "w_ge" else W > 0)
            h = (S / W[:, None]).astype(f32)
            nh = (N / W).astype(f32)
            n1 = np.fmin((nh + f32(1.0)).astype(f32), f32(max_history)).astype(f32)
            if mutant == "fmin_is_minimum":
                n1 = np.minimum((nh + f32(1.0)).astype(f32), f32(max_history)).astype(f32)
            elif mutant == "cap_after_add":
                n1 = (np.fmin(nh, f32(max_history)).astype(f32) + f32(1.0)).astype(f32)
            al = (f32(1.0) / n1).astype(f32)
            b = (h + (al[:, None] * (color - h).astype(f32)).astype(f32)).astype(f32)
            take = have & np.isfinite(b).all(axis=1)
        out[take] = b[take]
        nn[take] = n1[take]
        Wsum = np.where(ok, W, f32(0.0)).astype(f32)
    A = np.concatenate([out, nn[:, None]], axis=1).astype(f32)
    Nrm = np.concatenate([normal, np.zeros((n, 1), f32)], axis=1).astype(f32)
    res = (out, (A, rec.copy(), Nrm, obj.copy()))
    return res + (Wsum,) if want_taps else res


# ---- the G-buffer on the CPU: the oracle's camera and closest hit at the pixel centres -----------------------------------------------------
def frozen_world(wd, t):
    """A copy of the world with every closure-sequenced hitable parameter evaluated at time t in f32 (base + vel * t, a multiply and an
    add) and made constant: what the kernels see when every ray of a packet carries the time t."""
    import copy
    out = copy.deepcopy(wd) if not hasattr(wd, "_fields_") else type(wd).from_buffer_copy(wd)
    t = f32(t)
    for i in range(out.n_hitables):
        h = out.hitables[i]
        if h.animated:
            for c in ("x", "y", "z"):
                setattr(h.center, c, float(f32(f32(getattr(h.center, c)) + f32(f32(getattr(h.center_vel, c)) * t))))
                setattr(h.center_vel, c, 0.0)
            h.animated = 0
        if h.scale_vel != 0.0:
            h.scale = float(f32(f32(h.scale) + f32(f32(h.scale_vel) * t)))
            h.scale_vel = 0.0
    return out


def pixel_centre_rays(oracle, wd, p, fma=False):
    """(origins (n, 3), directions (n, 3)) of the G-buffer's rays: oracle probe_shading op 0 at uv = ndc * (pixel + 0.5), lens (0.5, 0.5), t0 = time_start."""
    W, H = int(p.width), int(p.height)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")  # pixel index x + y * W
    xs, ys = xs.reshape(-1).astype(f32), ys.reshape(-1).astype(f32)
    ndc_x, ndc_y = f32(f32(1.0) / f32(W)), f32(f32(1.0) / f32(H))
    inp = np.stack([(ndc_x * (xs + f32(0.5)).astype(f32)).astype(f32), (ndc_y * (ys + f32(0.5)).astype(f32)).astype(f32),
                    np.full(W * H, 0.5, f32), np.full(W * H, 0.5, f32), np.full(W * H, f32(p.time_start), f32)], axis=1)
    out = oracle.probe_shading(wd, 0, 0, inp, fma=fma)
    return out[:, :3].copy(), out[:, 3:].copy()


def gbuffer_oracle(oracle, wd, p, fma=False):
    """The G-buffer (records (n, 4), objects (n,)) of world wd under the frame parameters p from the CPU oracle: the rays above through
    oracle closest_hit at depth 0 on the world frozen at p.time_start (the oracle's probe marches at ray time 0), then P = o + t * d."""
    org, dirs = pixel_centre_rays(oracle, wd, p, fma)
    t, obj = oracle.closest_hit(frozen_world(wd, p.time_start), p, 0, org, dirs, fma=fma)
    return gbuffer_assemble(org, dirs, t, obj)


def world_hitables(wd):
    """[(animated, (vx, vy, vz))] of a world description, as accumulate() takes it"""
    return [(bool(wd.hitables[i].animated), (wd.hitables[i].center_vel.x, wd.hitables[i].center_vel.y, wd.hitables[i].center_vel.z)) for i in range(wd.n_hitables)]


# ---- a synthetic case whose arithmetic is exact: an axis-aligned orthographic camera over the plane z = 0 ---------------------------------
def ortho_camera(width, height, origin_x=0.0, pixel=0.125):
    """An _abi.Camera looking down -z from z = 4 with one pixel = `pixel` world units: for power-of-two sizes every basis vector, product
    and quotient of the projection is exact, so a point under a pixel centre reprojects to exactly that pixel."""
    from rayn_amd import _abi
    c = _abi.Camera()
    c.kind = _abi.CAM_ORTHOGRAPHIC
    c.res_w, c.res_h, c.vfov_or_size = float(width), float(height), pixel * height
    c.origin.x, c.origin.y, c.origin.z = origin_x, 0.0, 4.0
    c.at.x, c.at.y, c.at.z = origin_x, 0.0, 0.0
    c.up.x, c.up.y, c.up.z = 0.0, 1.0, 0.0
    return c


def ortho_plane_gbuffer(width, height, origin_x=0.0, pixel=0.125, obj=1):
    """The G-buffer that camera sees of the plane z = 0 (object `obj`), and the plane's film normal (0, 0, 1)"""
    xs, ys = np.meshgrid(np.arange(width), np.arange(height), indexing="xy")
    P = np.stack([(xs.reshape(-1) + 0.5 - width / 2) * pixel + origin_x, (ys.reshape(-1) + 0.5 - height / 2) * pixel, np.zeros(width * height)], axis=1)
    rec = np.concatenate([P, np.full((width * height, 1), 4.0)], axis=1).astype(f32)
    normal = np.tile(np.array([0.0, 0.0, 1.0], f32), (width * height, 1))
    return rec, np.full(width * height, obj, np.uint32), normal


# ---- the sequence the defaults of rayn_amd.Temporal were chosen on (tools/temporal_defaults.py, tests/test_temporal_device.py) -------------
class DefaultsCase:
    """The shipped scene at 160x96 under a camera whose origin moves (setup_s3's drift), 8 frames at samples=2, scored against samples=256."""
    W, H, FRAMES, SAMPLES, REF_SAMPLES, BOUNCES = 160, 96, list(range(1, 9)), 2, 256, 3

    @classmethod
    def scene(cls):
        """(world description, [frame params], reference frame params of the last frame)"""
        import rayn_amd as R
        from rayn_amd import setup as S
        from rayn_amd.scene import Linear
        cam, world = S.setup((cls.W, cls.H))
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(0.9, -0.3, 0.15))
        ps = [R.frame_params(cls.W, cls.H, cls.SAMPLES, cls.BOUNCES, frame=f) for f in cls.FRAMES]
        return world.to_desc(cam), ps, R.frame_params(cls.W, cls.H, cls.REF_SAMPLES, cls.BOUNCES, frame=cls.FRAMES[-1])

    @classmethod
    def mse(cls, color, background, want):
        """MSE of the saturated Color + Background against the saturated reference image `want`"""
        return float(np.mean((np.clip(np.asarray(color).reshape(cls.H, cls.W, 3).astype(np.float64) + np.asarray(background).reshape(cls.H, cls.W, 3), 0.0, 1.0) - want) ** 2))
