"""numpy restatement of the temporal supersampling (rayn_hip_temporal_upscale_device; the definition is in include/rayn_hip.h): the guided
upscaling's tiers on a footprint that may come from a projection through the low camera, the confidence of the value they give, and the
temporal accumulate at the high size with that confidence in its blend - binary32 operation by operation, tap by tap in the definition's
order; only the pixels are vectorised.  The camera projection (step 3 of the accumulate), its constants and the history layout are
imported from tests/temporal_np.py, expf from the oracle (denoise_np.oracle_expf); everything else is restated here.  It shares no code
with rayn_amd/csrc/temporal_upscale.hip.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this.

MUTANTS names the wrong readings of one decision each that tests/reproject_cases.py tells from the statement (temporal_upscale(...,
mutant=); mutant=None is the statement): the temporal predicates phase C shares with the accumulate, and the confidence rule where tier 1
added taps and still summed to Wg == 0 - `S.W > 0` fails, tier 2 gives the value, and conf is TIER 2's largest b."""
import numpy as np

from denoise_np import oracle_expf
from temporal_np import MISS, dot, project

f32 = np.float32
PLANES = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))
MUTANTS = ("depth_lt", "normal_gt", "ntap_gt", "te_ge",  # temporal_np's readings, in phase C
           "fmin_is_minimum",                            # n' = min(nh + conf, max_history) with a NaN nh propagating
           "conf_keeps_tier1")                           # conf stays tier 1's largest b when Wg == 0 sent the pixel to tier 2


def _origin(x0f):
    """step 4's integer tap origin: floorf clamped to [-2, 2^31] (a non-finite value never gets here: the projection rejects it)"""
    return np.clip(np.where(np.isfinite(x0f), x0f, f32(-2.0)), f32(-2.0), f32(2147483648.0)).astype(np.int64)


def footprint(width, height, factor, high_g, low_cam, time_start):
    """Step A: (fx, fy, projected) of every high pixel - the default footprint of the upscale, replaced by the projection of the pixel's
    primary hit through low_cam at time_start (at the LOW size) where there is a low camera, the pixel is a hit and the projection counts."""
    w, h, s = int(width), int(height), int(factor)
    W, H = w * s, h * s
    hrec, hobj = np.asarray(high_g[0], f32).reshape(W * H, 4), np.asarray(high_g[1]).reshape(W * H).astype(np.uint32)
    Xi, Yi = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    Xi, Yi = Xi.reshape(-1), Yi.reshape(-1)
    with np.errstate(all="ignore"):
        fx = (((Xi.astype(f32) + f32(0.5)).astype(f32) / f32(s)).astype(f32) - f32(0.5)).astype(f32)
        fy = (((Yi.astype(f32) + f32(0.5)).astype(f32) / f32(s)).astype(f32) - f32(0.5)).astype(f32)
        projected = np.zeros(W * H, bool)
        if low_cam is not None:
            ok, pfx, pfy, _ = project(low_cam, time_start, [hrec[:, 0], hrec[:, 1], hrec[:, 2]], w, h)
            projected = ok & (hobj != MISS)
            fx, fy = np.where(projected, pfx, fx).astype(f32), np.where(projected, pfy, fy).astype(f32)
    return fx, fy, projected


def temporal_upscale(film, low_g, high_g, width, height, factor, sigma_plane, sigma_position, low_cam, time_start, confidence, prev, prev_cam,
                     prev_time, hitables, max_history, depth_tolerance, normal_min, mutant=None):
    """One call.  film: the low film's planes ("color" and "normal" required, "alpha" / "background" optional), pixel x + y * width;
    low_g / high_g: (records, objects) of the G-buffers; low_cam: an _abi.Camera or None; prev: the previous HIGH history as (A, B, N, O)
    or None, with prev_cam and prev_time; hitables = [(animated, (vx, vy, vz))].  Returns (planes of the high film - "color" the
    ACCUMULATED colour, the others this frame's upscaled values -, weight (N,), new history (A', B', N', O'), info) with info = {"tier":
    1..3 per pixel, "conf", "frame_color": this frame's upscaled Color, "taps": the summed history tap weight (0 where the pixel reset
    before its taps), "n": the new history length, "projected": pixels whose footprint came from the projection, "rejected": history
    taps inside the image that failed a test}."""
    assert mutant is None or mutant in MUTANTS, mutant
    w, h, s = int(width), int(height), int(factor)
    W, H = w * s, h * s
    n, N = w * h, W * H
    src = {k: np.asarray(film[k], f32).reshape(n, c) for k, c in PLANES if film.get(k) is not None}
    lrec, lobj = np.asarray(low_g[0], f32).reshape(n, 4), np.asarray(low_g[1]).reshape(n).astype(np.uint32)
    hrec, hobj = np.asarray(high_g[0], f32).reshape(N, 4), np.asarray(high_g[1]).reshape(N).astype(np.uint32)
    sp, ss = f32(sigma_plane), f32(sigma_position)
    use_p, use_s = sigma_plane != 0, sigma_position != 0
    Xi, Yi = np.meshgrid(np.arange(W), np.arange(H), indexing="xy")
    Xi, Yi = Xi.reshape(-1), Yi.reshape(-1)
    fin_low = np.isfinite(src["color"]).all(axis=1)
    hit = hobj != MISS

    fx, fy, projected = footprint(w, h, s, high_g, low_cam, time_start)
    with np.errstate(all="ignore"):
        # ---- B: the three tiers on that footprint
        x0f, y0f = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        wx1, wy1 = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
        wx0, wy0 = (f32(1.0) - wx1).astype(f32), (f32(1.0) - wy1).astype(f32)
        x0, y0 = _origin(x0f), _origin(y0f)
        inv_t = (f32(1.0) / (hrec[:, 3] + f32(1e-8)).astype(f32)).astype(f32)
        kp = f32(f32(1.0) / f32(sp * sp)) if use_p else None
        ks = f32(f32(1.0) / f32(ss * ss)) if use_s else None

        def sums():
            return np.full(N, -0.0, f32), {k: np.full((N, v.shape[1]), -0.0, f32) for k, v in src.items()}, np.zeros(N, f32)

        def taps():
            for k in range(4):
                qx, qy = x0 + (k & 1), y0 + (k >> 1)
                inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
                q = np.where(inside, qx + qy * w, 0)
                b = ((wx1 if k & 1 else wx0) * (wy1 if k >> 1 else wy0)).astype(f32)
                yield q, b, inside & (b > 0) & fin_low[q]

        def add(use, g, b, q, Wt, St, bmax):
            Wt = np.where(use, (Wt + g).astype(f32), Wt).astype(f32)
            for key in St:
                St[key] = np.where(use[:, None], (St[key] + (g[:, None] * src[key][q]).astype(f32)).astype(f32), St[key]).astype(f32)
            return Wt, np.where(use, np.fmax(bmax, b), bmax).astype(f32)

        Wg, Sg, bg = sums()
        for q, b, usable in taps():
            d = [(hrec[:, c] - lrec[q, c]).astype(f32) for c in range(3)]
            e = np.zeros(N, f32)
            if use_p:
                nq = src["normal"][q]
                dpl = (np.abs(dot([nq[:, 0], nq[:, 1], nq[:, 2]], d)).astype(f32) * inv_t).astype(f32)
                e = ((dpl * dpl).astype(f32) * kp).astype(f32)
            if use_s:
                dps = (dot(d, d).astype(f32) * (inv_t * inv_t).astype(f32)).astype(f32)
                e = (e + (dps * ks).astype(f32)).astype(f32) if use_p else (dps * ks).astype(f32)
            g = np.where(hit, (b * oracle_expf((-e).astype(f32)).astype(f32)).astype(f32), b).astype(f32)
            Wg, bg = add(usable & (lobj[q] == hobj) & ~np.isnan(g), g, b, q, Wg, Sg, bg)
        Wb, Sb, bb = sums()
        for q, b, usable in taps():
            Wb, bb = add(usable, b, b, q, Wb, Sb, bb)
        t1 = Wg > 0
        t2 = ~t1 & (Wb > 0)
        t3 = ~(t1 | t2)
        qc = np.minimum(Xi // s, w - 1) + np.minimum(Yi // s, h - 1) * w
        frame = {}
        for key in src:
            a = np.where(t1[:, None], (Sg[key] / Wg[:, None]).astype(f32), (Sb[key] / Wb[:, None]).astype(f32)).astype(f32)
            a[t3] = src[key][qc][t3]  # verbatim: the float32 bits of the low film
            frame[key] = a
        weight = np.where(t1, Wg, f32(0.0)).astype(f32)
        conf = np.where(t1, bg, np.where(t2, bb, f32(1.0))).astype(f32) if confidence else np.ones(N, f32)
        if confidence and mutant == "conf_keeps_tier1":
            conf = np.where(t2 & (bg > 0), bg, conf).astype(f32)

        # ---- C: the accumulate at the high size, conf in step 5
        c, nrm = frame["color"], frame["normal"]
        cfin = np.isfinite(c).all(axis=1)
        out = c.copy()
        nn = np.where(cfin, f32(1.0), f32(0.0)).astype(f32)
        Wsum = np.zeros(N, f32)
        rejected = np.zeros(N, bool)
        go = cfin & hit
        if prev is not None and go.any():
            pA, pB, pN, pO = [np.asarray(a) for a in prev]
            pA, pB, pN, pO = pA.reshape(N, 4), pB.reshape(N, 4), pN.reshape(N, 4), pO.reshape(N)
            dt = f32(f32(time_start) - f32(prev_time))
            Pp = [hrec[:, k].copy() for k in range(3)]
            for k, (animated, vel) in enumerate(hitables):
                if animated:
                    m = hobj == k
                    for a in range(3):
                        Pp[a] = np.where(m, (hrec[:, a] - (f32(vel[a]) * dt).astype(f32)).astype(f32), Pp[a]).astype(f32)
            ok, hx, hy, te = project(prev_cam, prev_time, Pp, W, H, "te_ge" if mutant == "te_ge" else None)
            ok = ok & go
            X0f, Y0f = np.floor(hx).astype(f32), np.floor(hy).astype(f32)
            vx1, vy1 = (hx - X0f).astype(f32), (hy - Y0f).astype(f32)
            vx0, vy0 = (f32(1.0) - vx1).astype(f32), (f32(1.0) - vy1).astype(f32)
            X0, Y0 = _origin(X0f), _origin(Y0f)
            tol = (f32(depth_tolerance) * te).astype(f32)
            Wh, S, Nh = np.zeros(N, f32), np.zeros((N, 3), f32), np.zeros(N, f32)
            for k in range(4):
                qx, qy = X0 + (k & 1), Y0 + (k >> 1)
                inside = ok & (qx >= 0) & (qx < W) & (qy >= 0) & (qy < H)
                q = np.where(inside, qx + qy * W, 0)
                a = pA[q]
                dd = np.abs((pB[q, 3] - te).astype(f32))
                use = inside & (a[:, 3] > f32(1.0) if mutant == "ntap_gt" else a[:, 3] >= f32(1.0)) & (pO[q] == hobj)
                use &= dd < tol if mutant == "depth_lt" else dd <= tol
                if f32(normal_min) > f32(-1.0):
                    nq = pN[q]
                    dn = dot([nrm[:, 0], nrm[:, 1], nrm[:, 2]], [nq[:, 0], nq[:, 1], nq[:, 2]])
                    use &= dn > f32(normal_min) if mutant == "normal_gt" else dn >= f32(normal_min)
                rejected |= inside & ~use
                wt = ((vx1 if k & 1 else vx0) * (vy1 if k >> 1 else vy0)).astype(f32)
                Wh = np.where(use, (Wh + wt).astype(f32), Wh).astype(f32)
                for a_ in range(3):
                    S[:, a_] = np.where(use, (S[:, a_] + (wt * a[:, a_]).astype(f32)).astype(f32), S[:, a_])
                Nh = np.where(use, (Nh + (wt * a[:, 3]).astype(f32)).astype(f32), Nh).astype(f32)
            have = ok & (Wh > 0)
            hcol = (S / Wh[:, None]).astype(f32)
            nh = (Nh / Wh).astype(f32)
            n1 = (np.minimum if mutant == "fmin_is_minimum" else np.fmin)((nh + conf).astype(f32), f32(max_history)).astype(f32)
            al = (conf / n1).astype(f32)
            bl = (hcol + (al[:, None] * (c - hcol).astype(f32)).astype(f32)).astype(f32)
            take = have & np.isfinite(bl).all(axis=1)
            out[take] = bl[take]
            nn[take] = n1[take]
            Wsum = np.where(ok, Wh, f32(0.0)).astype(f32)
    A = np.concatenate([out, nn[:, None]], axis=1).astype(f32)
    Nrm = np.concatenate([nrm, np.zeros((N, 1), f32)], axis=1).astype(f32)
    planes = {"color": out}
    for key in src:
        if key != "color":
            planes[key] = frame[key] if frame[key].shape[1] == 3 else frame[key][:, 0]
    info = {"tier": np.where(t1, 1, np.where(t2, 2, 3)).astype(np.uint8), "conf": conf, "frame_color": c, "taps": Wsum, "n": nn,
            "projected": projected, "rejected": rejected}
    return planes, weight, (A, hrec.copy(), Nrm, hobj.copy()), info
