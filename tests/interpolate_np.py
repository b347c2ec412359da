"""numpy restatement of the frame generation (rayn_hip_interpolate_device; the definition is in include/rayn_hip.h), binary32 operation by
operation, written from the header text.  It reuses the projection (step 3 of the temporal accumulate), the camera constants and the f32
helpers of tests/temporal_np.py and shares no code with rayn_amd/csrc/interpolate.hip; tests/test_interpolate_device.py compares the two
bit for bit.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this.

MUTANTS names the wrong readings of one decision each that tests/reproject_cases.py tells from the statement (interpolate(..., mutant=);
mutant=None is the statement).  "zc_ge" (temporal_np.EQUIVALENT) is accepted and is no mutant here either: the frame generation uses the
same projection, whose finiteness test rejects zc = 0 whatever the sign test said (the pinhole and thin-lens keys of
reproject_cases.interpolate_from_accumulate put zc at 0 and one ulp either side of it)."""
import numpy as np

from restatement_np import f32
from temporal_np import MISS, ortho_camera, ortho_plane_gbuffer, project

PLANES = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))
NEG_ZERO = f32(-0.0)
MUTANTS = ("weight_ge",    # a tap of bilinear weight b == 0 is used (b >= 0)
           "te_ge",        # orthographic: a point on a key camera's plane is accepted, through the shared projection
           "depth_lt",     # |t_tap - te| < tol
           "tie_takes_b")  # tier 2 with neither own pixel usable: wA > wB, so B is taken at the exact half
EQUIVALENT = ("zc_ge",)


class Key:
    """One key frame: film = {plane: array} (color required; alpha / background / normal optional), rec (n, 4), obj (n,), the _abi.Camera
    it was rendered through and its time_start."""

    def __init__(self, film, rec, obj, camera, time_start):
        self.film, self.rec, self.obj, self.camera, self.time = film, rec, obj, camera, time_start


def _planes(film, n):
    return {k: np.asarray(film[k], f32).reshape(n, c) for k, c in PLANES if film.get(k) is not None}


def _gather(key, width, height, rec, obj, ts, hitables, depth_tolerance, mutant=None):
    """Steps 1 and 2 for one key: (W (n,), {plane: S (n, c)})."""
    n = width * height
    film = _planes(key.film, n)
    krec, kobj = np.asarray(key.rec, f32).reshape(n, 4), np.asarray(key.obj, np.uint32).reshape(n)
    hit = obj != MISS
    xs, ys = np.meshgrid(np.arange(width), np.arange(height), indexing="xy")
    with np.errstate(all="ignore"):
        dt = f32(f32(ts) - f32(key.time))
        Pp = [rec[:, c].copy() for c in range(3)]
        for k, (animated, vel) in enumerate(hitables):
            if animated:
                m = obj == k
                for c in range(3):
                    Pp[c] = np.where(m, (rec[:, c] - (f32(vel[c]) * dt).astype(f32)).astype(f32), Pp[c]).astype(f32)
        ok, fx, fy, te = project(key.camera, key.time, Pp, width, height, mutant if mutant in ("te_ge", "zc_ge") else None)
        ok = np.where(hit, ok, True)
        fx = np.where(hit, fx, xs.reshape(-1).astype(f32)).astype(f32)
        fy = np.where(hit, fy, ys.reshape(-1).astype(f32)).astype(f32)
        x0f, y0f = np.floor(fx).astype(f32), np.floor(fy).astype(f32)
        wx1, wy1 = (fx - x0f).astype(f32), (fy - y0f).astype(f32)
        wx0, wy0 = (f32(1.0) - wx1).astype(f32), (f32(1.0) - wy1).astype(f32)
        x0 = np.clip(np.where(np.isfinite(x0f), x0f, f32(-2.0)), f32(-2.0), f32(2147483648.0)).astype(np.int64)
        y0 = np.clip(np.where(np.isfinite(y0f), y0f, f32(-2.0)), f32(-2.0), f32(2147483648.0)).astype(np.int64)
        tol = (f32(depth_tolerance) * te).astype(f32)
        W = np.full(n, NEG_ZERO, f32)
        S = {k: np.full(v.shape, NEG_ZERO, f32) for k, v in film.items()}
        for k in range(4):
            qx, qy = x0 + (k & 1), y0 + (k >> 1)
            b = ((wx1 if k & 1 else wx0) * (wy1 if k >> 1 else wy0)).astype(f32)
            inside = ok & (qx >= 0) & (qx < width) & (qy >= 0) & (qy < height)
            q = np.where(inside, qx + qy * width, 0)
            use = inside & (b >= 0 if mutant == "weight_ge" else b > 0) & (kobj[q] == obj)
            dd = np.abs((krec[q, 3] - te).astype(f32))
            use &= np.where(hit, dd < tol if mutant == "depth_lt" else dd <= tol, True)
            use &= np.isfinite(film["color"][q]).all(axis=1)
            W = np.where(use, (W + b).astype(f32), W).astype(f32)
            for name, v in film.items():
                S[name] = np.where(use[:, None], (S[name] + (b[:, None] * v[q]).astype(f32)).astype(f32), S[name]).astype(f32)
    return W, S


def interpolate(width, height, key_a, key_b, rec, obj, ts, hitables, depth_tolerance, mutant=None):
    """One generated frame: ({plane: (n, c) array} for the planes of the keys' films, source (n,) uint32).  rec (n, 4), obj (n,): the
    frame's own G-buffer at time ts; hitables = [(animated, (vx, vy, vz))] of the world."""
    assert mutant is None or mutant in MUTANTS + EQUIVALENT, mutant
    n = width * height
    rec, obj = np.asarray(rec, f32).reshape(n, 4), np.asarray(obj, np.uint32).reshape(n)
    fa, fb = _planes(key_a.film, n), _planes(key_b.film, n)
    assert set(fa) == set(fb) and "color" in fa
    with np.errstate(all="ignore"):
        s = f32(f32(f32(ts) - f32(key_a.time)) / f32(f32(key_b.time) - f32(key_a.time)))
        wB = s
        wA = f32(f32(1.0) - s)
        WA, SA = _gather(key_a, width, height, rec, obj, ts, hitables, depth_tolerance, mutant)
        WB, SB = _gather(key_b, width, height, rec, obj, ts, hitables, depth_tolerance, mutant)
        validA, validB = WA > 0, WB > 0
        tier1 = validA | validB
        usableA, usableB = np.isfinite(fa["color"]).all(axis=1), np.isfinite(fb["color"]).all(axis=1)
        neither = ~usableA & ~usableB
        a_wins = wA > wB if mutant == "tie_takes_b" else wA >= wB
        # which keys a pixel takes its value from
        useA = np.where(tier1, validA, np.where(neither, a_wins, usableA))
        useB = np.where(tier1, validB, np.where(neither, ~a_wins, usableB))
        source = np.where(tier1, np.where(validA & validB, 0, np.where(validA, 1, 2)), np.where(usableA & usableB, 3, 4)).astype(np.uint32)
        out = {}
        for name in fa:
            vA = np.where(tier1[:, None], (SA[name] / WA[:, None]).astype(f32), fa[name])
            vB = np.where(tier1[:, None], (SB[name] / WB[:, None]).astype(f32), fb[name])
            mix = ((vA * wA).astype(f32) + (vB * wB).astype(f32)).astype(f32)
            out[name] = np.where((useA & useB)[:, None], mix, np.where(useA[:, None], vA, vB)).astype(f32)
    return out, source


def ortho_case(width, height, seed=1, pixel=0.125):
    """The exact synthetic case (power-of-two sizes): two keys whose orthographic cameras stand one pixel to the left (A) and one to the
    right (B) of the generated frame's, over the plane z = 0 (object 1, t = 4): the point under T's pixel x is under A's pixel x + 1 and
    under B's pixel x - 1, exactly.  Every plane is random; ta = 0, tb = 1.  -> (key A, key B, T's records, T's objects)."""
    rng = np.random.default_rng(seed)
    n = width * height
    keys = []
    films = [{"color": rng.random((n, 3)).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
              "normal": rng.normal(size=(n, 3)).astype(f32)} for _ in range(2)]
    for film, ox, t in zip(films, (-pixel, pixel), (0.0, 1.0)):
        rec, obj, _ = ortho_plane_gbuffer(width, height, origin_x=ox, pixel=pixel)
        keys.append(Key(film, rec, obj, ortho_camera(width, height, origin_x=ox, pixel=pixel), t))
    rec, obj, _ = ortho_plane_gbuffer(width, height, pixel=pixel)
    return keys[0], keys[1], rec, obj


# ---- the sequence the frame generation is measured on (tools/interpolate_defaults.py, tests/test_interpolate_device.py) --------------------
class InterpCase:
    """temporal_np.DefaultsCase's scene and size (the shipped scene at 160x96, samples=2, scored against samples=256) under three times its
    camera drift, (2.7, -0.9, 0.45) per second: at 24 frames a second the image moves about 2 pixels a frame, so 4 and 8 pixels between the
    keys of every = 2 and 4.  Frames 1..5: every = 2 renders 1, 3, 5 and generates 2, 4; every = 4 renders 1, 5 and generates 2, 3, 4."""
    DRIFT, FRAMES, RATE = (2.7, -0.9, 0.45), [1, 2, 3, 4, 5], 24

    @classmethod
    def scene(cls, samples):
        """(world description, {frame: frame params at `samples`})"""
        import rayn_amd as R
        from rayn_amd import setup as S
        from rayn_amd.scene import Linear
        from temporal_np import DefaultsCase as D
        cam, world = S.setup((D.W, D.H))
        c = world.cameras.get(cam)
        c.origin = Linear(c.origin, R.vec3(*cls.DRIFT))
        ps = {}
        for f in cls.FRAMES:
            start = f32(f) * (f32(1.0) / f32(cls.RATE))
            ps[f] = R.frame_params(D.W, D.H, samples, D.BOUNCES, frame=f, time_range=(float(start), float(f32(start + f32(1.0 / cls.RATE)))))
        return world.to_desc(cam), ps

    @staticmethod
    def keys_of(every):
        """[(generated frame, key A's frame, key B's frame)] of FRAMES under Interpolate(every)"""
        fr = InterpCase.FRAMES
        keys = [i for i in range(len(fr)) if i % every == 0 or i == len(fr) - 1]
        return [(fr[i], fr[max(k for k in keys if k < i)], fr[min(k for k in keys if k > i)]) for i in range(len(fr)) if i not in keys]

    @staticmethod
    def cross_fade(film_a, film_b, ta, tb, ts):
        """The plain cross-fade of two keys' Color and Background (tier 2 everywhere): a * wA + b * wB in f32."""
        s = f32(f32(f32(ts) - f32(ta)) / f32(f32(tb) - f32(ta)))
        wA, wB = f32(f32(1.0) - s), s
        return {k: ((np.asarray(film_a[k], f32) * wA).astype(f32) + (np.asarray(film_b[k], f32) * wB).astype(f32)).astype(f32) for k in ("color", "background")}
