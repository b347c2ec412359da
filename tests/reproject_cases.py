"""The reprojection post-process entries at their decision edges: named cases on the exact orthographic set-up of temporal_np.ortho_camera /
ortho_plane_gbuffer (camera at z = 4 over the plane z = 0, one pixel = 0.125: te is exactly 4, and with depth_tolerance 0.25 the depth
bound is exactly 1), each with the pixels under test and the outcome written out by hand - "at the bound, one ulp inside, one ulp
outside" wherever a comparison has two sides.  An accumulate case carries n' and whether the pixel blended, a Catmull-Rom case the arm, an
upscale case the tier, an interpolation case the source code; every pixel that is not under test is a control with the case's normal
outcome.  Every accumulate family runs at 16x8 (one block) and 32x16 (two); the projection and border families run through the
interpolation as well (interpolate_from_accumulate).  `kills` names the mutants ("T:depth_lt": temporal_np's; TR temporal_resample_np, TU temporal_upscale_np, U upscale_np,
I interpolate_np) whose result differs from the statement's on a pixel under test.  tests/test_reproject_cases.py holds all of this to
account without a GPU; tests/test_reproject_edges_device.py pushes every case through every kernel it applies to.
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

import interpolate_np as I
from common import above, below  # noqa: F401 (the tests reach them as RC.above / RC.below)
import temporal_np as T
import temporal_resample_np as TR
import temporal_upscale_np as TU
import upscale_np as U

f32 = np.float32
PIXEL = 0.125
INF, NAN = f32(np.inf), f32(np.nan)
MODULES = {"T": T, "TR": TR, "TU": TU, "U": U, "I": I}
UNKNOWN = -1  # an outcome the case does not write down


class Case:
    def __init__(self, name, entry, kills, **fields):
        self.name, self.entry, self.kills = name, entry, tuple(kills)
        self.__dict__.update(fields)

    def __repr__(self):
        return self.name


# ---- the accumulate family -----------------------------------------------------------------------------------------------------------------
class _Acc:
    """The exact set-up under construction: a current frame and a history of length 2 seen by a previous camera `shift` pixels away, so
    that pixel (x, y) reprojects to exactly (x + shift[0], y + shift[1]); every control pixel blends to n' = 3 (max_history 8)."""

    def __init__(self, w=16, h=8, shift=(0.0, 0.0), seed=1, tp=(8, 0.25, -1.0), kind=None, length=2.0):
        self.w, self.h, self.tp, n = w, h, tp, w * h
        rng = np.random.default_rng(seed)
        self.rec, self.obj, self.normal = T.ortho_plane_gbuffer(w, h)
        self.cam = T.ortho_camera(w, h, origin_x=-shift[0] * PIXEL)
        self.cam.origin.y = self.cam.at.y = -shift[1] * PIXEL
        if kind is not None:
            self.cam.kind, self.cam.vfov_or_size = kind, 53.0
        self.color = (0.25 + 0.5 * rng.random((n, 3))).astype(f32)
        self.A = np.concatenate([0.25 + 0.5 * rng.random((n, 3)), np.full((n, 1), length)], axis=1).astype(f32)
        self.B = self.rec.copy()
        self.N = np.concatenate([self.normal, np.zeros((n, 1), f32)], axis=1)
        self.O = self.obj.copy()
        self.M = (0.25 + 0.5 * rng.random((n, 2))).astype(f32)
        self.test = np.zeros(n, bool)
        self.n1 = np.full(n, min(length + 1.0, tp[0]), f32)
        self.blended = np.ones(n, np.int8)

    def p(self, x, y):
        return x + y * self.w

    def expect(self, p, n1, blended=None):
        """pixel p is under test: n' and whether it blended (default: n' > 1)"""
        self.test[p], self.n1[p] = True, n1
        self.blended[p] = (n1 > 1) if blended is None else blended

    def case(self, name, kills, entry="accumulate", **more):
        return Case(name, entry, kills, w=self.w, h=self.h, color=self.color, normal=self.normal, rec=self.rec, obj=self.obj,
                    prev=(self.A, self.B, self.N, self.O), mom=self.M, prev_cam=self.cam, tp=self.tp, test=self.test, n1=self.n1,
                    blended=self.blended, **more)


SHARED = ("depth_lt", "normal_gt", "ntap_gt", "te_ge", "fmin_is_minimum")  # the readings temporal_upscale_np shares with temporal_np


def _kills(*names):
    """the mutants of temporal_np, and of temporal_upscale_np where phase C has the same decision"""
    return tuple(f"T:{m}" for m in names) + tuple(f"TU:{m}" for m in names if m in SHARED)


def _spread(a, k):
    """k pixels of the interior, no two of them neighbours"""
    return [a.p(2 + 3 * (i % ((a.w - 3) // 3)), 1 + 2 * (i // ((a.w - 3) // 3))) for i in range(k)]


def depth_cases(w, h):
    out = []
    a = _Acc(w, h, seed=2)
    for p, (d, n1) in zip(_spread(a, 9), ((5.0, 3), (above(5.0), 1), (3.0, 3), (below(3.0), 1), (below(5.0), 3), (above(3.0), 3), (NAN, 1), (INF, 1), (-INF, 1))):
        a.B[p, 3] = d
        a.expect(p, n1)
    out.append(a.case(f"depth/bound/{w}x{h}", _kills("depth_lt")))
    a = _Acc(w, h, seed=3, tp=(8, 0.0, -1.0))
    for p, (d, n1) in zip(_spread(a, 4), ((4.0, 3), (above(4.0), 1), (below(4.0), 1), (NAN, 1))):
        a.B[p, 3] = d
        a.expect(p, n1)
    out.append(a.case(f"depth/tol0/{w}x{h}", _kills("depth_lt")))
    return out


def normal_cases(w, h):
    out = []
    a = _Acc(w, h, seed=4, tp=(8, 0.25, float(f32(0.8))))
    for p, (nz, n1) in zip(_spread(a, 5), ((f32(0.8), 3), (above(0.8), 3), (below(0.8), 1), (NAN, 1), (-INF, 1))):
        a.N[p, :3] = (0.0, 0.6, nz)  # against the film normal (0, 0, 1) the dot product is exactly nz
        a.expect(p, n1)
    out.append(a.case(f"normal/floor/{w}x{h}", _kills("normal_gt")))
    # the switch: at exactly -1 the test is off and a NaN history normal still counts; one ulp above it is on
    a = _Acc(w, h, seed=5, tp=(8, 0.25, -1.0))
    for p, (nrm, n1) in zip(_spread(a, 3), (((NAN, NAN, NAN), 3), ((0.0, 0.0, -1.0), 3), ((0.0, 0.0, -INF), 3))):
        a.N[p, :3] = nrm
        a.expect(p, n1)
    out.append(a.case(f"normal/switch_off/{w}x{h}", _kills("normal_switch_ge")))
    on = float(above(-1.0))
    a = _Acc(w, h, seed=6, tp=(8, 0.25, on))
    # a dot of exactly -1 lies BELOW nextafter(-1, 0) and is rejected; a dot of exactly the floor counts
    for p, (nrm, n1) in zip(_spread(a, 4), (((NAN, NAN, NAN), 1), ((0.0, 0.0, -1.0), 1), ((0.0, 0.0, on), 3), ((0.0, 0.0, above(on)), 3))):
        a.N[p, :3] = nrm
        a.expect(p, n1)
    out.append(a.case(f"normal/switch_on/{w}x{h}", _kills("normal_gt")))
    return out


def length_cases(w, h):
    a = _Acc(w, h, seed=7)
    for p, (n, n1) in zip(_spread(a, 8), ((1.0, 2), (below(1.0), 1), (0.5, 1), (0.0, 1), (-0.0, 1), (-1.0, 1), (NAN, 1), (above(1.0), above(1.0) + f32(1.0)))):
        a.A[p, 3] = n
        a.expect(p, n1)
    # +inf: on its own pixel the tap has weight 1, N = inf and n' is the cap; the three pixels that see it as a tap of weight 0 get
    # N = 0 * inf = NaN, and fminf gives the cap as well (blend/cap has the same pixel beside the other blend edges)
    q = a.p(8, 6)
    a.A[q, 3] = INF
    for p in (q, q - 1, q - a.w, q - a.w - 1):
        a.expect(p, 8)
    return [a.case(f"length/floor/{w}x{h}", _kills("ntap_gt"))]


def blend_cases(w, h):
    out = []
    a = _Acc(w, h, seed=8)
    for p, (n, n1) in zip(_spread(a, 4), ((7.0, 8), (6.5, 7.5), (7.5, 8), (below(7.0), below(7.0) + f32(1.0)))):
        a.A[p, 3] = n
        a.expect(p, n1)
    # an infinite length: on its own pixel the tap has weight 1 (N = inf, n' = max_history); for the three pixels that see it as a tap
    # of weight 0, N = 0 * inf is NaN and fminf returns max_history
    q = a.p(8, 5)
    a.A[q, 3] = INF
    for p in (q, q - 1, q - a.w, q - a.w - 1):
        a.expect(p, 8)
    # a NaN colour on a tap of weight 0 counts too: S = 0 * NaN, the blend is not finite and the pixel resets
    q = a.p(12, 5)
    a.A[q, 0] = NAN
    for p in (q, q - 1, q - a.w, q - a.w - 1):
        a.expect(p, 1)
    # history 3e38 against colour -3e38: c - h overflows, the blend is not finite
    q = a.p(4, 6)
    a.A[q, :3], a.color[q] = 3.0e38, -3.0e38
    a.expect(q, 1)
    # with moments: the colour blends, y * y overflows, (y, y2) is stored
    q = overflow = a.p(14, 1)
    a.A[q, :3], a.color[q] = 2.0e38, 2.0e38
    a.expect(q, 3, UNKNOWN)  # h == c: the blend has the colour's bits
    # a colour that is not finite: n' = 0
    for q, c in ((a.p(1, 6), NAN), (a.p(14, 6), INF)):
        a.color[q, 1] = c
        a.expect(q, 0, False)
    out.append(a.case(f"blend/cap/{w}x{h}", _kills("cap_after_add", "fmin_is_minimum", "zero_weight_skipped", "reset_keeps_length"),
                      moments_overflow=overflow))
    a = _Acc(w, h, seed=9, tp=(1, 0.25, -1.0))
    a.n1[:] = 1.0
    a.blended[:] = UNKNOWN  # a = 1: out = h + (c - h), which may round to c
    for p, n in zip(_spread(a, 3), (1.0, 5.0, INF)):
        a.A[p, 3] = n
        a.expect(p, 1, UNKNOWN)
    out.append(a.case(f"blend/max_history_1/{w}x{h}", _kills("cap_after_add")))
    # nh = 2^24, where nh + 1 == nh: the entries refuse a max_history above 65536 (check_temporal_params), so the absorbed sum can only
    # ever meet the cap - n' = 65536 - and the case pins that an nh far above the cap is clamped to it, not that the sum is absorbed
    a = _Acc(w, h, seed=10, tp=(65536, 0.25, -1.0))
    for p, (n, n1) in zip(_spread(a, 4), ((2.0 ** 24, 65536), (65535.0, 65536), (65534.5, 65535.5), (65536.0, 65536))):
        a.A[p, 3] = n
        a.expect(p, n1)
    out.append(a.case(f"blend/max_history_65536/{w}x{h}", _kills("cap_after_add")))
    return out


def object_cases(w, h):
    a = _Acc(w, h, seed=11)
    ps = _spread(a, 6)
    for p, o in zip(ps[:2], (0, 15)):
        a.obj[p] = a.O[p] = o
        a.expect(p, 3)
    a.O[ps[2]] = T.MISS  # a history miss under a hit pixel
    a.expect(ps[2], 1)
    a.obj[ps[3]], a.rec[ps[3]] = T.MISS, (0.0, 0.0, 0.0, INF)  # a current miss over a history hit
    a.expect(ps[3], 1)
    a.obj[ps[4]], a.rec[ps[4]], a.O[ps[4]] = T.MISS, (0.0, 0.0, 0.0, INF), T.MISS  # and over a history miss
    a.expect(ps[4], 1)
    a.obj[ps[5]], a.O[ps[5]] = 0, 15
    a.expect(ps[5], 1)
    return [a.case(f"object/ids/{w}x{h}", ())]


def projection_cases(w, h):
    out = []
    # a point exactly on the camera plane z = 4: te = (qx * wx + qy * wy) + 0 * -1 with wx = wy = +0 is +0; a camera whose `at` has
    # x = y = -0.0 has wx = wy = -0 and te = -0, every other value unchanged.  The history depth is set to te: only project() decides.
    a = _Acc(w, h, seed=17)
    a.cam.origin.x = a.cam.origin.y = 0.0
    a.cam.at.x = a.cam.at.y = -0.0
    for p in (a.p(2, 1), a.p(12, 6)):
        a.rec[p, 2], a.B[p, 3] = 4.0, 0.0
        a.expect(p, 1)
    out.append(a.case(f"projection/ortho_negative_zero/{w}x{h}", _kills("te_ge"), zero_te=np.array([a.p(2, 1), a.p(12, 6)]), te_sign=True))
    a = _Acc(w, h, seed=12)
    for p in (a.p(2, 1), a.p(12, 6)):
        a.rec[p, 2], a.B[p, 3] = 4.0, 0.0
        a.expect(p, 1)
    p = a.p(5, 3)  # one ulp in front of the plane
    a.rec[p, 2] = below(4.0)
    a.B[p, 3] = f32(4.0) - below(4.0)
    a.expect(p, 3)
    p = a.p(8, 3)  # and one ulp behind it
    a.rec[p, 2] = above(4.0)
    a.B[p, 3] = f32(4.0) - above(4.0)
    a.expect(p, 1)
    for p, (c, v) in zip((a.p(11, 3), a.p(2, 5), a.p(5, 5), a.p(8, 5), a.p(11, 1), a.p(14, 3)),
                         ((0, 3.0e38), (1, 3.0e38), (0, NAN), (2, NAN), (1, -3.0e38), (0, INF))):
        a.rec[p, c] = v  # fx or fy overflows with te = 4, or a position that is not finite
        a.expect(p, 1)
    out.append(a.case(f"projection/ortho/{w}x{h}", _kills("te_ge"), zero_te=np.array([a.p(2, 1), a.p(12, 6)]), te_sign=False))
    # the perspective cameras at (0, 0, 4) looking down -z: every current point lies on the axis, projects to (w / 2 - 0.5, h / 2 - 0.5)
    # and has te = zc = 4 - Pz; depth_tolerance 1e30 takes the depth test out, so that only project() decides
    for kind in (0, 1):
        a = _Acc(w, h, seed=13 + kind, tp=(8, 1e30, -1.0), kind=kind)
        a.rec[:, :3] = 0.0
        for p, (z, n1) in zip(_spread(a, 6), ((4.0, 1), (below(4.0), 3), (above(4.0), 1), (3.0, 3), (5.0, 1), (NAN, 1))):
            a.rec[p, 2] = z
            a.expect(p, n1)
        out.append(a.case(f"projection/{'pinhole' if kind == 0 else 'thin_lens'}/{w}x{h}", ()))
    return out


def _solve(cam, w, h, axis, target):
    """The coordinate (x for axis 0, y for axis 1) of a point of the plane z = 0 whose projection lands on exactly fx (fy) == target: the
    analytic value, then its float neighbours on the restatement.  None when no float does."""
    target = f32(target)
    ox = f32(cam.origin.x) if axis == 0 else f32(cam.origin.y)
    size = (w, h)[axis]
    guess = (np.float64(target) + 0.5) * PIXEL - size * PIXEL / 2 + np.float64(ox)
    v = f32(guess)
    cands = [v]
    lo = hi = v
    for _ in range(8):
        lo, hi = np.nextafter(lo, -INF), np.nextafter(hi, INF)
        cands += [lo, hi]
    for v in cands:
        P = [np.array([v if axis == 0 else 0.0], f32), np.array([v if axis == 1 else 0.0], f32), np.zeros(1, f32)]
        got = T.project(cam, 0.0, P, w, h)[1 + axis][0]
        if got.view(np.uint32) == target.view(np.uint32):
            return v
    return None


def border_targets(size, which):
    """(f, does a tap of weight > 0 lie inside?) around the low border, the high border, or at both (the corners) of an axis of `size`"""
    low = ((-1.0, False), (above(-1.0), True), (-0.5, True), (0.0, True))
    high = ((size - 1.0, True), (above(size - 1.0), True), (size - 0.5, True), (float(size), False))
    return {"low": low, "high": high, "corners": (low[0], low[2], high[2], high[3])}[which]


def border_cases(w, h):
    """fx and fy at and around the borders, through the current G-buffer's positions (each exact in f32: asserted by _solve on the
    restatement): every value of one axis with the other in the middle, then every pair.  nextabove(-1) is not reachable with the camera
    at 0 - fx's last rounding swallows it - so the low border's camera stands where ll = (0.0625, 0.0625) and q = P - ll is exact to
    2^-28; nextabove(size - 1) is reachable only from 0.  fx = -0.0 is not reachable at all (uvx * width - 0.5 is -0 for no uvx);
    +0.0 stands in for it.  fx == -1 and fx == size leave taps of weight 0 inside at most: W = 0, a reset."""
    out = []
    for which in ("low", "high", "corners"):
        a = _Acc(w, h, seed=15)
        if which == "low":
            a.cam.origin.x = a.cam.at.x = w * PIXEL / 2 + PIXEL / 2
            a.cam.origin.y = a.cam.at.y = h * PIXEL / 2 + PIXEL / 2
        xs, ys = border_targets(w, which), border_targets(h, which)
        sol_x = [_solve(a.cam, w, h, 0, t) for t, _ in xs]
        sol_y = [_solve(a.cam, w, h, 1, t) for t, _ in ys]
        assert all(v is not None for v in sol_x + sol_y), (which, sol_x, sol_y)
        a.rec[:, 0], a.rec[:, 1] = _solve(a.cam, w, h, 0, 3.0), _solve(a.cam, w, h, 1, 2.0)  # the controls all land on history pixel (3, 2)
        ps = iter(range(a.w + 1, a.w * a.h - 1))
        for i, (_, inx) in enumerate(xs):
            p = next(ps)
            a.rec[p, 0] = sol_x[i]
            a.expect(p, 3 if inx else 1)
        for j, (_, iny) in enumerate(ys):
            p = next(ps)
            a.rec[p, 1] = sol_y[j]
            a.expect(p, 3 if iny else 1)
        for i, (_, inx) in enumerate(xs):
            for j, (_, iny) in enumerate(ys):
                p = next(ps)
                a.rec[p, 0], a.rec[p, 1] = sol_x[i], sol_y[j]
                a.expect(p, 3 if inx and iny else 1)
        out.append(a.case(f"border/{which}/{w}x{h}", _kills("tap_inside_le") if which != "low" else (), targets=(xs, ys)))
    return out


def tiny_cases():
    """1x1 and 3x3: no Catmull-Rom footprint fits; 3x3 is not a power of two, so only the centre pixel's zero shift is exact"""
    out = []
    for w in (1, 3):
        a = _Acc(w, w, seed=16)
        a.n1[:], a.blended[:] = np.nan, UNKNOWN
        a.expect(a.p(w // 2, w // 2), 3)
        out.append(a.case(f"tiny/{w}x{w}", (), "tiny", arm=np.where(a.test, TR.ARM_BILINEAR, UNKNOWN).astype(np.int8), not_cubic=True))
    return out


ACCUMULATE_FAMILIES = (depth_cases, normal_cases, length_cases, blend_cases, object_cases, projection_cases, border_cases)


# ---- Catmull-Rom: the arm ------------------------------------------------------------------------------------------------------------------
def _interior(w, h):
    """pixels whose 4x4 footprint lies in the image under a (0.5, 0.5) shift: x0 = x, 1 <= x0 and x0 + 2 <= w - 1"""
    xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    return ((xs >= 1) & (xs <= w - 3) & (ys >= 1) & (ys <= h - 3)).reshape(-1)


def _sees(w, h, tx, ty):
    """pixels whose footprint holds the tap (tx, ty), and those whose bilinear 2x2 does"""
    xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
    xs, ys = xs.reshape(-1), ys.reshape(-1)
    return (xs - 1 <= tx) & (tx <= xs + 2) & (ys - 1 <= ty) & (ty <= ys + 2), (xs <= tx) & (tx <= xs + 1) & (ys <= ty) & (ty <= ys + 1)


def catmull_rom_cases():
    out = []
    w, h = 16, 8
    inner = _interior(w, h)
    base_arm = np.where(inner, TR.ARM_CUBIC, TR.ARM_BILINEAR).astype(np.int8)

    def acc(seed, tp=(8, 0.25, -1.0), **kw):
        a = _Acc(w, h, shift=(0.5, 0.5), seed=seed, tp=tp, **kw)
        a.n1[:], a.blended[:] = np.nan, 1
        a.case = lambda name, kills, _case=a.case, **more: _case(name, kills, "resample", **more)
        return a

    # the footprint rule at the borders: x0 == 1 and x0 + 2 == w - 1 are inside, x0 == 0 and x0 + 2 == w are outside
    a = acc(20)
    a.test[:] = True
    out.append(a.case("catmull_rom/footprint", ("TR:footprint_le",), arm=base_arm))
    a = _Acc(32, 16, shift=(0.5, 0.5), seed=19)  # more than one block
    a.n1[:], a.test[:] = np.nan, True
    out.append(a.case("catmull_rom/footprint/32x16", ("TR:footprint_le",), "resample", arm=np.where(_interior(32, 16), TR.ARM_CUBIC, TR.ARM_BILINEAR).astype(np.int8)))
    a = _Acc(4, 4, shift=(0.5, 0.5), seed=21)
    a.n1[:], a.test[:] = np.nan, True
    out.append(a.case("catmull_rom/4x4", ("TR:footprint_le",), "resample", arm=np.where(_interior(4, 4), TR.ARM_CUBIC, TR.ARM_BILINEAR).astype(np.int8)))
    # exactly one of the sixteen taps at each predicate's edge: at the bound the cubic arm, one ulp beyond the bilinear one
    tx, ty = 6, 4
    sees, sees2 = _sees(w, h, tx, ty)
    q = tx + ty * w
    for name, kill, tp, edits in (("depth", "depth_lt", (8, 0.25, -1.0), ((5.0, True), (above(5.0), False), (3.0, True), (below(3.0), False))),
                                  ("normal", "normal_gt", (8, 0.25, float(f32(0.8))), ((f32(0.8), True), (below(0.8), False))),
                                  ("length", "ntap_gt", (8, 0.25, -1.0), ((1.0, True), (below(1.0), False)))):
        for i, (v, counts) in enumerate(edits):
            a = acc(22 + i, tp)
            if name == "depth":
                a.B[q, 3] = v
            elif name == "normal":
                a.N[q, :3] = (0.0, 0.6, v)
            else:
                a.A[q, 3] = v
            a.test[:] = sees & inner
            arm = base_arm.copy()
            if not counts:
                arm[sees & inner] = TR.ARM_BILINEAR  # every 2x2 has four taps of weight 0.25: where the tap is one of them, three are left
            out.append(a.case(f"catmull_rom/{name}/{'at' if counts else 'beyond'}{i}", (f"TR:{kill}",) if counts else (), arm=arm))
    # the anti-ringing clamp: a constant history resamples to exactly lo == hi; a spike on an outer tap undershoots and is clamped
    a = acc(30)
    a.A[:, :3] = 0.75
    a.test[:] = inner
    out.append(a.case("catmull_rom/clamp_on_lo_and_hi", (), arm=base_arm, resampled=0.75))
    # lo < hi: the history varies by column only (the rows' weights sum to exactly 1), and with t = 0.5 the columns weigh (-1, 9, 9, -1) / 16.
    # Columns 5..8 = (4, 1, 2, 7) resample to (27 - 11) / 16 = 1 == lo of the inner (1, 2) at x = 6; columns 10..13 = (-2, 1, 2, -3) to
    # (27 + 5) / 16 = 2 == hi at x = 11; every product and sum is exact, so the clamp is handed v == lo and v == hi with lo < hi.
    a = acc(33)
    a.A[:, :3] = 1.5
    for x, v in zip((5, 6, 7, 8, 10, 11, 12, 13), (4.0, 1.0, 2.0, 7.0, -2.0, 1.0, 2.0, -3.0)):
        a.A[x::w, :3] = v
    at_lo, at_hi = np.array([a.p(6, y) for y in range(1, h - 2)]), np.array([a.p(11, y) for y in range(1, h - 2)])
    a.test[at_lo] = a.test[at_hi] = True
    out.append(a.case("catmull_rom/clamp_at_lo_and_at_hi", (), arm=base_arm, at_lo=at_lo, at_hi=at_hi, lo=1.0, hi=2.0))
    a = acc(31)
    a.A[:, :3] = 0.75
    a.A[q, :3] = 100.0
    a.test[:] = sees & ~sees2 & inner
    out.append(a.case("catmull_rom/clamp_changes", ("TR:clamp_outer",), arm=base_arm, clamped_to=0.75))
    # lengths whose weighted mean falls below 1: the inner four are 1, the outer twelve 5 -> 1.265625 - 0.265625 * 5 < 0, floored to 1
    a = acc(32, length=5.0)
    p = a.p(6, 3)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1)):
        a.A[p + dx + dy * w, 3] = 1.0
    a.expect(p, 2)
    out.append(a.case("catmull_rom/length_floor", ("TR:length_unfloored",), arm=base_arm))
    return out


# ---- the upscale's tiers -------------------------------------------------------------------------------------------------------------------
def _upscale_base(w, h, s, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    lrec, lobj, nrm = T.ortho_plane_gbuffer(w, h)
    hrec, hobj, _ = T.ortho_plane_gbuffer(w * s, h * s, pixel=PIXEL / s)
    film = {"color": (0.25 + 0.5 * rng.random((n, 3))).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
            "normal": nrm.copy()}
    return film, [lrec, lobj], [hrec, hobj]


def _high_of(w, s, lx, ly):
    """the s x s high pixels of the low pixel (lx, ly)"""
    return np.array([(lx * s + i) + (ly * s + j) * w * s for j in range(s) for i in range(s)])


def upscale_cases():
    out = []
    w, h, s = 16, 8, 2
    N = w * h * s * s

    def case(name, kills, film, low_g, high_g, sigmas, test, tier, **more):
        return Case(name, "upscale", kills, w=w, h=h, factor=more.pop("factor", s), film=film, low_g=tuple(low_g), high_g=tuple(high_g), sigmas=sigmas,
                    test=test, tier=tier, **more)

    # every matching tap's weight underflows to exactly 0 (the nearest tap has e = 1.2e-4 / 1e-8 >> 104): Wg == 0, tier 2
    film, lg, hg = _upscale_base(w, h, s, 40)
    out.append(case("upscale/underflow", ("U:tier1_any_match", "U:tier2_skipped"), film, lg, hg, (0.0, 1e-4), np.ones(N, bool), np.full(N, 2, np.uint8)))
    # the same with the nearest tap of the pixels of low pixel (5, 3) showing another object: tier 1 would have b <= 0.1875, tier 2's
    # largest b is 0.5625 - the confidence is tier 2's
    film, lg, hg = _upscale_base(w, h, s, 41)
    lg[1][5 + 3 * w] = 2
    test = np.zeros(N, bool)
    test[_high_of(w, s, 5, 3)] = True
    out.append(case("upscale/underflow_confidence", ("TU:conf_keeps_tier1",), film, lg, hg, (0.0, 1e-4), test, np.full(N, 2, np.uint8), conf=0.5625))
    # a denormal weight: e = 95 on the nearest tap (every other tap underflows), Wg = 0.5625 * expf(-95) > 0: tier 1
    film, lg, hg = _upscale_base(w, h, s, 42)
    dps = f32(f32(2 * 0.03125 ** 2) * f32(f32(1.0) / f32(f32(4.0) + f32(1e-8))) ** 2)
    sigma = float(np.sqrt(float(dps) / 95.0))
    out.append(case("upscale/denormal_weight", (), film, lg, hg, (0.0, sigma), np.ones(N, bool), np.full(N, 1, np.uint8), denormal=True))
    # a NaN weight: the plane term of a low tap at x = inf is |0 * -inf + ...| = NaN; the tap is skipped, the other three give tier 1
    film, lg, hg = _upscale_base(w, h, s, 43)
    lg[0][6 + 4 * w, 0] = INF
    test = np.zeros(N, bool)
    for lx in (5, 6):
        for ly in (3, 4):
            test[_high_of(w, s, lx, ly)] = True
    out.append(case("upscale/nan_weight", ("U:nan_weight_counts",), film, lg, hg, (0.02, 0.0), test, np.full(N, 1, np.uint8)))
    # every tap not finite: tier 3, the low pixel verbatim
    film, lg, hg = _upscale_base(w, h, s, 44)
    test = np.zeros(N, bool)
    for lx in (8, 9, 10):
        for ly in (2, 3, 4):
            film["color"][lx + ly * w, (lx + ly) % 3] = (NAN, INF, -INF)[(lx + ly) % 3]
    test[_high_of(w, s, 9, 3)] = True
    tier = np.full(N, 1, np.uint8)
    tier[_high_of(w, s, 9, 3)] = 3
    tier[[i for lx in (8, 9, 10) for ly in (2, 3, 4) if (lx, ly) != (9, 3) for i in _high_of(w, s, lx, ly)]] = 0  # not written down
    out.append(case("upscale/all_taps_dead", (), film, lg, hg, (0.02, 0.05), test, tier))
    # factor 1: every footprint is integral - one tap of weight 1, three of weight 0 that are skipped; an inf Alpha on a neighbour stays out
    film, lg, hg = _upscale_base(w, h, 1, 45)
    film["alpha"][7 + 3 * w] = INF
    test = np.zeros(w * h, bool)
    test[[6 + 3 * w, 7 + 2 * w, 6 + 2 * w]] = True
    out.append(case("upscale/zero_weight_tap", ("U:weight_ge",), film, lg, hg, (0.02, 0.05), test, np.full(w * h, 1, np.uint8), factor=1, finite_alpha=True))
    return out


# ---- the interpolation ---------------------------------------------------------------------------------------------------------------------
def interpolate_cases():
    out = []
    W, H = 32, 16
    n = W * H
    px = lambda x, y: x + y * W

    def case(name, kills, ka, kb, rec, obj, ts, tol, test, source):
        return Case(name, "interpolate", kills, w=W, h=H, ka=ka, kb=kb, rec=rec, obj=obj, ts=ts, tol=tol, test=test, source=source)

    def controls():
        # A stands one pixel left and B one right: pixel x reads A's x + 1 and B's x - 1, so the border columns have one key only
        src = np.zeros((H, W), np.uint32)
        src[:, 0], src[:, W - 1] = 1, 2
        return src.reshape(-1)

    # the depth bound on key B's tap (te = 4, tol = 1), ts at both keys and halfway
    for ts in (0.0, 0.5, 1.0):
        ka, kb, rec, obj = I.ortho_case(W, H, 50)
        src, test = controls(), np.zeros(n, bool)
        for y, (d, ok) in enumerate(((5.0, True), (above(5.0), False), (3.0, True), (below(3.0), False), (NAN, False)), 2):
            kb.rec[px(24, y), 3] = d  # read by pixel x = 25
            test[px(25, y)], src[px(25, y)] = True, 0 if ok else 1
        out.append(case(f"interpolate/depth/ts{ts}", ("I:depth_lt",), ka, kb, rec, obj, ts, 0.25, test, src))
    # a point on both key cameras' plane, the keys' depths set to te = 0: the projection alone rejects it, tier 2 cross-fades (source 3)
    ka, kb, rec, obj = I.ortho_case(W, H, 51)
    src, test = controls(), np.zeros(n, bool)
    for p in (px(6, 3), px(20, 12)):
        rec[p, 2] = 4.0
        ka.rec[p + 1, 3] = kb.rec[p - 1, 3] = 0.0
        test[p], src[p] = True, 3  # (the edited taps have weight 1 for p alone; for every other pixel their weight is 0 and they are skipped)
    out.append(case("interpolate/on_the_camera_plane", ("I:te_ge",), ka, kb, rec, obj, 0.5, 0.25, test, src))
    # tier 2 with both own pixels not finite at ts exactly halfway: source 4, and A is taken (wA >= wB)
    ka, kb, rec, obj = I.ortho_case(W, H, 52)
    src, test = controls(), np.zeros(n, bool)
    p = px(10, 7)
    obj[p] = 7  # no key shows it: no tap counts
    ka.film["color"][p, 0], kb.film["color"][p, 2] = NAN, INF
    test[p], src[p] = True, 4
    q = px(15, 7)
    obj[q] = 7
    kb.film["color"][q, 1] = NAN  # one own pixel usable: A's, also source 4
    test[q], src[q] = True, 4
    # a key pixel that is not finite is also a dead tap for the pixel that reads it: x - 1 reads A's x, x + 1 reads B's x
    for r, code in ((p - 1, 2), (p + 1, 1), (q + 1, 1)):
        test[r], src[r] = True, code
    out.append(case("interpolate/tie_takes_a", ("I:tie_takes_b",), ka, kb, rec, obj, 0.5, 0.25, test, src))
    out[-1].takes_a = np.array([p, q])
    # the taps of weight 0 (every footprint is integral) are skipped: an inf Alpha beside the tap of weight 1 stays out
    ka, kb, rec, obj = I.ortho_case(W, H, 53)
    src, test = controls(), np.zeros(n, bool)
    ka.film["alpha"][px(13, 5)] = INF  # A's tap of weight 1 for x = 12; of weight 0 for x = 11 and the row below
    for p in (px(11, 5), px(11, 4), px(12, 4)):
        test[p] = True
    out.append(case("interpolate/zero_weight_tap", ("I:weight_ge",), ka, kb, rec, obj, 0.5, 0.25, test, src))
    out[-1].finite_alpha = True
    return out


def interpolate_border_cases():
    """The x borders through two keys that see them differently (interpolate_from_accumulate has both axes, the corners and the
    nextabove values through two keys that stand together): the frame's points are placed so that key A (one pixel to the left: B's fx is A's - 2)
    sees them at fx = -1, -0.5, 0 (B: outside) and at w - 1, w - 0.5, w (B: inside).  At fx == -1 A's only tap inside has weight 0 and is
    skipped: neither key counts, tier 2 cross-fades the own pixels (source 3); at fx == w only B counts (2)."""
    W, H = 32, 16
    ka, kb, rec, obj = I.ortho_case(W, H, 54)
    src, test = np.zeros(W * H, np.uint32), np.zeros(W * H, bool)
    rec[:, 0] = _solve(ka.camera, W, H, 0, 4.0)  # the controls: A's pixel 4, B's pixel 2
    targets = ((-1.0, 3), (-0.5, 1), (0.0, 1), (1.0, 1), (W - 1.0, 0), (W - 0.5, 0), (float(W), 2))
    for p, (t, code) in zip(range(W + 3, W * H, 37), targets):
        x = _solve(ka.camera, W, H, 0, t)
        assert x is not None and _solve(kb.camera, W, H, 0, f32(t) - f32(2.0)) == x, t
        rec[p, 0], test[p], src[p] = x, True, code
    return [Case("interpolate/border_one_key", "interpolate", (), w=W, h=H, ka=ka, kb=kb, rec=rec, obj=obj, ts=0.25, tol=0.25, test=test, source=src)]


SIZES = ((16, 8), (32, 16))  # one 16x16 block; two


def interpolate_from_accumulate(c, seed=55):
    """An accumulate case of the projection or border family as an interpolation case: BOTH keys stand at the case's previous camera and
    carry its history's depths and objects, the frame is the case's current G-buffer.  Every such pixel blends (n' == 3) exactly when a
    tap of weight > 0 is inside and passes - the interpolation's rule too, which skips the taps of weight 0 the accumulate counts - so
    both keys count (source 0); where the accumulate resets, neither does and tier 2 cross-fades the two own pixels (source 3)."""
    assert c.name.startswith(("projection/", "border/")) and set(np.unique(c.n1).tolist()) <= {1.0, 3.0}
    rng = np.random.default_rng(seed)
    n = c.w * c.h
    keys = [I.Key({"color": rng.random((n, 3)).astype(f32), "alpha": rng.random(n).astype(f32), "background": rng.random((n, 3)).astype(f32),
                   "normal": rng.normal(size=(n, 3)).astype(f32)}, c.prev[1].copy(), c.prev[3].copy(), c.prev_cam, t) for t in (0.0, 1.0)]
    kills = ("I:te_ge",) if "T:te_ge" in c.kills else ()
    more = {k: getattr(c, k) for k in ("zero_te", "te_sign", "targets") if hasattr(c, k)}
    return Case("interpolate/" + c.name, "interpolate", kills, w=c.w, h=c.h, ka=keys[0], kb=keys[1], rec=c.rec, obj=c.obj, ts=0.5, tol=c.tp[1],
                test=c.test, source=np.where(c.n1 == 3, 0, 3).astype(np.uint32), perspective=c.prev_cam.kind != 2, **more)


def accumulate_cases():
    return [c for fam in ACCUMULATE_FAMILIES for w, h in SIZES for c in fam(w, h)] + tiny_cases()


def all_cases():
    acc = accumulate_cases()
    derived = [interpolate_from_accumulate(c) for c in acc if c.name.startswith(("projection/", "border/"))]
    return acc + catmull_rom_cases() + upscale_cases() + interpolate_cases() + interpolate_border_cases() + derived


# ---- running a case on a restatement -------------------------------------------------------------------------------------------------------
def run_accumulate(c, mutant=None, want_taps=False):
    """temporal_np.accumulate -> (out, history[, W])"""
    return T.accumulate(c.w, c.h, c.color, c.normal, c.rec, c.obj, c.prev, c.prev_cam, 0.0, 0.0, [], *c.tp, want_taps=want_taps, mutant=mutant)


def run_resample(c, resample, moments=False, mutant=None, want_unclamped=False):
    """temporal_resample_np.accumulate -> (out, history, moments, arm[, unclamped])"""
    return TR.accumulate(c.w, c.h, c.color, c.normal, c.rec, c.obj, c.prev, c.mom if moments else None, c.prev_cam, 0.0, 0.0, [], *c.tp, resample,
                         want_unclamped=want_unclamped, mutant=mutant)


def run_temporal_upscale_1(c, mutant=None):
    """an accumulate case through temporal_upscale_np at factor 1, no low camera, confidence off -> (planes, weight, history, info)"""
    return TU.temporal_upscale({"color": c.color, "normal": c.normal}, (c.rec, c.obj), (c.rec, c.obj), c.w, c.h, 1, 0.0, 0.0, None, 0.0, False, c.prev,
                               c.prev_cam, 0.0, [], *c.tp, mutant=mutant)


def run_upscale(c, mutant=None):
    """upscale_np.upscale -> (planes, weight, tier, emax)"""
    return U.upscale(c.film, c.low_g, c.high_g, c.w, c.h, c.factor, *c.sigmas, mutant=mutant)


def upscale_history(c, seed=60):
    """a previous high history (length 2, the high G-buffer's own records) and its camera for an upscale case through the supersampling"""
    W, H = c.w * c.factor, c.h * c.factor
    rng = np.random.default_rng(seed)
    hrec, hobj = c.high_g
    A = np.concatenate([0.25 + 0.5 * rng.random((W * H, 3)), np.full((W * H, 1), 2.0)], axis=1).astype(f32)
    N = np.concatenate([np.tile(np.array([0.0, 0.0, 1.0], f32), (W * H, 1)), np.zeros((W * H, 1), f32)], axis=1)
    return (A, np.asarray(hrec, f32).copy(), N, np.asarray(hobj, np.uint32).copy()), T.ortho_camera(W, H, pixel=PIXEL / c.factor)


def run_temporal_upscale(c, confidence, mutant=None, tp=(8, 0.25, -1.0)):
    """an upscale case through temporal_upscale_np with upscale_history -> (planes, weight, history, info)"""
    prev, cam = upscale_history(c)
    return TU.temporal_upscale(c.film, c.low_g, c.high_g, c.w, c.h, c.factor, *c.sigmas, None, 0.0, confidence, prev, cam, 0.0, [], *tp, mutant=mutant)


def run_interpolate(c, mutant=None):
    """interpolate_np.interpolate -> (planes, source)"""
    return I.interpolate(c.w, c.h, c.ka, c.kb, c.rec, c.obj, c.ts, [], c.tol, mutant=mutant)
