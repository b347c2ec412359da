"""numpy restatement of the temporal accumulate with a choice of the history resampling filter (rayn_hip_temporal_accumulate_resample_device;
the definition is in include/rayn_hip.h), binary32 operation by operation.  Steps 1 - 3 and 5 and the bilinear arm are temporal_np's and
temporal_variance_np's; the Catmull-Rom arm of step 4 is written here from the definition and shares no code with rayn_amd/csrc.
tests/test_temporal_resample_device.py compares the kernels with it bit for bit.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this.

MUTANTS names wrong readings of the Catmull-Rom arm alone (accumulate(..., mutant=), without moments; mutant=None is the statement): the
bilinear arm and steps 1 - 3 stay temporal_np's unmutated ones, which is the drift the kernel's two copies of the predicate are free to
take.  tests/reproject_cases.py has the cases that tell each from the statement."""
import numpy as np

import temporal_np as T
import temporal_variance_np as TV

f32 = np.float32
MISS = T.MISS
ARM_RESET, ARM_BILINEAR, ARM_CUBIC = 0, 1, 2
MUTANTS = ("depth_lt",          # the footprint's copy of the predicate: |t_tap - te| < tol
           "normal_gt",         # its dot(nrm, nrm_tap) > normal_min
           "ntap_gt",           # its n_tap > 1
           "footprint_le",      # x0 < 0, x0 + 2 > width (and y): a footprint one pixel over the border counts, read from the clamped pixel
           "clamp_outer",       # the anti-ringing range over all 16 taps
           "length_unfloored")  # nh = N / W without the fmaxf(., 1)


def cubic_weights(t):
    """The Catmull-Rom weights of the offsets -1, 0, 1, 2 at the fraction t (an f32 array), every product and sum rounded to f32"""
    t = np.asarray(t, f32)
    with np.errstate(all="ignore"):
        def m(a, b):
            return (a * b).astype(f32)

        def a_(a, b):
            return (a + b).astype(f32)
        km = m(a_(m(a_(m(f32(-0.5), t), f32(1.0)), t), f32(-0.5)), t)
        k0 = a_(m(m(a_(m(f32(1.5), t), f32(-2.5)), t), t), f32(1.0))
        k1 = m(a_(m(a_(m(f32(-1.5), t), f32(2.0)), t), f32(0.5)), t)
        k2 = m(m(a_(m(f32(0.5), t), f32(-0.5)), t), t)
    return [km, k0, k1, k2]


def fminf(a, b):
    """fminf as the definition takes it: the other operand for a NaN, and -0 below +0"""
    a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
    r = np.fmin(a, b).astype(f32)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, (a.view(np.uint32) | b.view(np.uint32)).view(f32), r).astype(f32)


def fmaxf(a, b):
    a, b = np.broadcast_arrays(np.asarray(a, f32), np.asarray(b, f32))
    r = np.fmax(a, b).astype(f32)
    zeros = (a == 0) & (b == 0)
    return np.where(zeros, (a.view(np.uint32) & b.view(np.uint32)).view(f32), r).astype(f32)


def clamp(v, lo, hi):
    return fminf(fmaxf(v, lo), hi)


def accumulate(width, height, color, normal, rec, obj, prev, prev_moments, prev_cam, prev_time, cur_time, hitables, max_history, depth_tolerance,
               normal_min, resample, want_unclamped=False, mutant=None):
    """One temporal accumulate through the resample entry.  Arguments as temporal_variance_np.accumulate (prev_moments None and prev given:
    no moments, as temporal_np.accumulate), plus resample (0 bilinear, 1 Catmull-Rom) and `moments` implied by prev_moments / with_moments.
    Returns (out colour (n, 3), (A', B', N', O'), moments (n, 2) or None, arm (n,)): arm 0 the pixel reset, 1 it blended the bilinear taps,
    2 it blended the Catmull-Rom footprint.  With want_unclamped also the cubic arm's h before the anti-ringing clamp ((n, 3); NaN
    outside arm 2)."""
    return _accumulate(width, height, color, normal, rec, obj, prev, prev_moments, prev_moments is not None, prev_cam, prev_time, cur_time, hitables,
                       max_history, depth_tolerance, normal_min, resample, want_unclamped, mutant)


def accumulate_first(width, height, color, normal, rec, obj, with_moments, max_history=4, depth_tolerance=0.05, normal_min=-1.0, resample=0):
    """The first frame of a sequence: no previous history, every pixel resets"""
    return _accumulate(width, height, color, normal, rec, obj, None, None, with_moments, None, 0.0, 0.0, [], max_history, depth_tolerance, normal_min,
                       resample, False)


def _accumulate(width, height, color, normal, rec, obj, prev, prev_moments, with_moments, prev_cam, prev_time, cur_time, hitables, max_history,
                depth_tolerance, normal_min, resample, want_unclamped, mutant=None):
    assert resample in (0, 1) and (mutant is None or (mutant in MUTANTS and not with_moments))
    n = width * height
    # the bilinear result everywhere: steps 1 - 5 of the existing definitions
    if with_moments:
        out, hist, mom = TV.accumulate(width, height, color, normal, rec, obj, prev, prev_moments, prev_cam, prev_time, cur_time, hitables, max_history,
                                       depth_tolerance, normal_min)
        Wsum = None if prev is None else T.accumulate(width, height, color, normal, rec, obj, prev, prev_cam, prev_time, cur_time, hitables, max_history,
                                                      depth_tolerance, normal_min, want_taps=True)[2]
    else:
        res = T.accumulate(width, height, color, normal, rec, obj, prev, prev_cam, prev_time, cur_time, hitables, max_history, depth_tolerance, normal_min,
                           want_taps=True)
        out, hist, mom, Wsum = res[0], res[1], None, res[2]
    color = np.asarray(color, f32).reshape(n, 3)
    normal = np.asarray(normal, f32).reshape(n, 3)
    rec, obj = np.asarray(rec, f32).reshape(n, 4), np.asarray(obj, np.uint32).reshape(n)
    A = hist[0]
    # a pixel whose new history is what a reset writes (out = c, n' = 1, or 0 for a non-finite c) is a reset: a blend that lands on exactly
    # those bits cannot be told from one, and does not need to be
    reset_like = (out.view(np.uint32) == color.view(np.uint32)).all(axis=1) & (A[:, 3] <= f32(1.0))
    arm = np.where((Wsum > 0) & ~reset_like, ARM_BILINEAR, ARM_RESET).astype(np.int8) if prev is not None else np.zeros(n, np.int8)
    unclamped = np.full((n, 3), np.nan, f32)
    if resample == 0 or prev is None:
        return (out, hist, mom, arm) + ((unclamped,) if want_unclamped else ())
    pA, pB, pN, pO = [np.asarray(a) for a in prev]
    pA, pB, pN, pO = pA.reshape(n, 4), pB.reshape(n, 4), pN.reshape(n, 4), pO.reshape(n)
    pM = np.asarray(prev_moments, f32).reshape(n, 2) if with_moments else None
    cfin = np.isfinite(color).all(axis=1)
    with np.errstate(all="ignore"):
        # steps 2 and 3
        dt = f32(f32(cur_time) - f32(prev_time))
        Pp = [rec[:, c].copy() for c in range(3)]
        for k, (animated, vel) in enumerate(hitables):
            if animated:
                for c in range(3):
                    Pp[c] = np.where(obj == k, (rec[:, c] - (f32(vel[c]) * dt).astype(f32)).astype(f32), Pp[c]).astype(f32)
        ok, fx, fy, te = T.project(prev_cam, prev_time, Pp, width, height)
        ok = ok & cfin & (obj != MISS)
        # step 4, the Catmull-Rom arm
        x0f, y0f = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        tx, ty = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
        x0 = np.where(np.isfinite(x0f), np.clip(x0f, -2.0, 2.0 ** 31), -2.0).astype(np.int64)
        y0 = np.where(np.isfinite(y0f), np.clip(y0f, -2.0, 2.0 ** 31), -2.0).astype(np.int64)
        tol = (f32(depth_tolerance) * te).astype(f32)
        kx, ky = cubic_weights(tx), cubic_weights(ty)
        full = ok.copy()
        W, N, S1, S2 = (np.zeros(n, f32) for _ in range(4))
        S = np.zeros((n, 3), f32)
        inner = []
        for j in range(-1, 3):
            for i in range(-1, 3):
                qx, qy = x0 + i, y0 + j
                counts = ok & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
                q = np.where(counts, qx + qy * width, 0)
                if mutant == "footprint_le":
                    counts = ok & (x0 >= 0) & (x0 + 2 <= width) & (y0 >= 0) & (y0 + 2 <= height)
                    q = np.where(counts, np.clip(qx, 0, width - 1) + np.clip(qy, 0, height - 1) * width, 0)
                dd = np.abs((pB[q, 3] - te).astype(f32))
                counts &= pA[q, 3] > f32(1.0) if mutant == "ntap_gt" else pA[q, 3] >= f32(1.0)
                counts &= pO[q] == obj
                counts &= dd < tol if mutant == "depth_lt" else dd <= tol
                if f32(normal_min) > f32(-1.0):
                    dn = T.dot([normal[:, 0], normal[:, 1], normal[:, 2]], [pN[q, 0], pN[q, 1], pN[q, 2]])
                    counts &= dn > f32(normal_min) if mutant == "normal_gt" else dn >= f32(normal_min)
                full &= counts
                w = (kx[i + 1] * ky[j + 1]).astype(f32)
                W = (W + w).astype(f32)
                for c in range(3):
                    S[:, c] = (S[:, c] + (w * pA[q, c]).astype(f32)).astype(f32)
                N = (N + (w * pA[q, 3]).astype(f32)).astype(f32)
                if with_moments:
                    S1 = (S1 + (w * pM[q, 0]).astype(f32)).astype(f32)
                    S2 = (S2 + (w * pM[q, 1]).astype(f32)).astype(f32)
                if (i in (0, 1) and j in (0, 1)) or mutant == "clamp_outer":
                    inner.append(q)
        h = (S / W[:, None]).astype(f32)
        unclamped[full] = h[full]
        nh = (N / W).astype(f32) if mutant == "length_unfloored" else fmaxf((N / W).astype(f32), f32(1.0))

        def ranged(v, plane, c):
            lo, hi = plane[inner[0], c], plane[inner[0], c]
            for q in inner[1:]:
                lo, hi = fminf(lo, plane[q, c]), fmaxf(hi, plane[q, c])
            return clamp(v, lo, hi)

        h = np.stack([ranged(h[:, c], pA, c) for c in range(3)], axis=1)
        # step 5
        n1 = np.fmin((nh + f32(1.0)).astype(f32), f32(max_history)).astype(f32)
        a = (f32(1.0) / n1).astype(f32)
        blend = (h + (a[:, None] * (color - h).astype(f32)).astype(f32)).astype(f32)
        take = full & np.isfinite(blend).all(axis=1)
        gone = full & ~take  # a non-finite blend resets the pixel
        if with_moments:
            y = TV.luminance(color)
            y2 = (y * y).astype(f32)
            h1, h2 = ranged((S1 / W).astype(f32), pM, 0), ranged((S2 / W).astype(f32), pM, 1)
            m1 = (h1 + (a * (y - h1).astype(f32)).astype(f32)).astype(f32)
            m2 = (h2 + (a * (y2 - h2).astype(f32)).astype(f32)).astype(f32)
            mtake = take & np.isfinite(m1) & np.isfinite(m2)
    out, A = out.copy(), A.copy()
    out[take], A[take, :3], A[take, 3] = blend[take], blend[take], n1[take]
    out[gone], A[gone, :3], A[gone, 3] = color[gone], color[gone], f32(1.0)
    arm[take], arm[gone] = ARM_CUBIC, ARM_RESET
    if with_moments:
        mom = mom.copy()
        mom[full] = np.stack([y, y2], axis=1)[full]
        mom[mtake] = np.stack([m1, m2], axis=1)[mtake]
    return (out, (A, hist[1], hist[2], hist[3]), mom, arm) + ((unclamped,) if want_unclamped else ())
