"""The Catmull-Rom history resample of the temporal accumulate without a GPU: the numpy restatement (tests/temporal_resample_np.py) against
the existing restatements and against the properties its definition promises, Temporal(resample=) validation, and the ABI struct."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import temporal_np as T
import temporal_resample_cases as K
import temporal_resample_np as TR
import temporal_variance_np as TV
from common import bits_equal

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIT = K.moving_world()[1]  # the hitables of the world the GPU test uploads: object 1 moves


def _ortho_case(w, h, sx, sy, seed, lengths=(1.0, 2.0, 3.5)):
    """The exact orthographic case of test_temporal_device: a previous camera sx / sy pixels aside over the plane z = 0, every tap valid"""
    rng = np.random.default_rng(seed)
    n = w * h
    rec, obj, normal = T.ortho_plane_gbuffer(w, h)
    prev_cam = T.ortho_camera(w, h, origin_x=-sx * 0.125)
    prev_cam.origin.y = prev_cam.at.y = -sy * 0.125
    prev_rec, _, _ = T.ortho_plane_gbuffer(w, h, origin_x=-sx * 0.125)
    prev_rec[:, 1] -= f32(sy * 0.125)
    A = np.concatenate([rng.random((n, 3)), rng.choice(np.array(lengths), n)[:, None]], axis=1).astype(f32)
    prev = (A, prev_rec, np.concatenate([normal, np.zeros((n, 1), f32)], axis=1), obj)
    return prev_cam, rng.random((n, 3)).astype(f32), normal, rec, obj, prev, rng.random((n, 2)).astype(f32)


@pytest.mark.parametrize("cam_kind", [0, 1, 2])
def test_resample_0_is_the_existing_restatements_bit_for_bit(cam_kind):
    pc, c, nr, rec, obj, prev, M = K.adversarial_inputs(5 + cam_kind, cam_kind)
    for nm in (-1.0, 0.8):
        out, hist, mom, arm = TR.accumulate(K.W, K.H, c, nr, rec, obj, prev, None, pc, K.PREV_TIME, K.CUR_TIME, HIT, 8, 0.05, nm, 0)
        want = T.accumulate(K.W, K.H, c, nr, rec, obj, prev, pc, K.PREV_TIME, K.CUR_TIME, HIT, 8, 0.05, nm)
        assert mom is None and bits_equal(out, want[0]) and all(bits_equal(a, b) for a, b in zip(hist[:3], want[1][:3])) and np.array_equal(hist[3], want[1][3])
        out, hist, mom, arm = TR.accumulate(K.W, K.H, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, K.CUR_TIME, HIT, 8, 0.05, nm, 0)
        want = TV.accumulate(K.W, K.H, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, K.CUR_TIME, HIT, 8, 0.05, nm)
        assert bits_equal(out, want[0]) and all(bits_equal(a, b) for a, b in zip(hist[:3], want[1][:3])) and bits_equal(mom, want[2])
        assert not (arm == TR.ARM_CUBIC).any() and (arm == TR.ARM_BILINEAR).any() and (arm == TR.ARM_RESET).any()


@pytest.mark.parametrize("cam_kind", [0, 1, 2])
@pytest.mark.parametrize("normal_min", [-1.0, 0.8])
def test_the_adversarial_case_reaches_every_arm(cam_kind, normal_min):
    """The condition the GPU test asserts before it compares: the restatement alone sends at least 25 % of the pixels down the cubic arm,
    15 % down the bilinear fallback and 5 % into a reset."""
    pc, c, nr, rec, obj, prev, M = K.adversarial_inputs(5 + cam_kind, cam_kind)
    arm = TR.accumulate(K.W, K.H, c, nr, rec, obj, prev, M, pc, K.PREV_TIME, K.CUR_TIME, HIT, 8, 0.05, normal_min, 1)[3]
    shares = K.arm_shares(arm)
    assert all(shares[code] >= least for code, least in K.MIN_SHARE.items()), shares


def test_integral_reprojections_return_the_tap():
    """fx and fy integers: t = 0, the weights are (-0, 1, 0, +-0), W = 1 and the cubic arm returns the tap's colour, length and moments as
    values - the sign of a zero may differ - which is also what the bilinear arm returns."""
    w, h = 16, 8
    for sx, sy in ((0.0, 0.0), (3.0, 0.0), (0.0, 2.0), (-2.0, 1.0)):
        pc, c, nr, rec, obj, prev, M = _ortho_case(w, h, sx, sy, 3)
        cub = TR.accumulate(w, h, c, nr, rec, obj, prev, M, pc, 0.0, 0.0, [], 64, 0.05, 0.9, 1, want_unclamped=True)
        lin = TR.accumulate(w, h, c, nr, rec, obj, prev, M, pc, 0.0, 0.0, [], 64, 0.05, 0.9, 0)
        two = cub[3] == TR.ARM_CUBIC
        assert two.sum() >= (w - 3 - abs(sx)) * (h - 3 - abs(sy)) and (lin[3][two] == TR.ARM_BILINEAR).all()
        assert np.array_equal(cub[0], lin[0]) and np.array_equal(cub[1][0], lin[1][0]) and np.array_equal(cub[2], lin[2])
        xs, ys = np.meshgrid(np.arange(w), np.arange(h), indexing="xy")
        tap = ((xs + int(sx)) + (ys + int(sy)) * w).reshape(-1)[two]  # the previous camera sits sx pixels to the left
        assert np.array_equal(cub[4][two], prev[0][tap, :3])             # h before the clamp is the tap's colour
        assert np.array_equal(cub[1][0][two, 3], prev[0][tap, 3] + f32(1.0))  # n' = n_tap + 1 below the cap


def test_a_3x5_image_never_takes_the_cubic_arm():
    for w, h in ((3, 5), (5, 3), (3, 2)):
        pc, c, nr, rec, obj, prev, M = _ortho_case(w, h, 0.25, -0.5, 4)
        cub = TR.accumulate(w, h, c, nr, rec, obj, prev, M, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 1)
        lin = TR.accumulate(w, h, c, nr, rec, obj, prev, M, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 0)
        assert not (cub[3] == TR.ARM_CUBIC).any() and (cub[3] == TR.ARM_BILINEAR).any()
        assert bits_equal(cub[0], lin[0]) and bits_equal(cub[1][0], lin[1][0]) and bits_equal(cub[2], lin[2])


def test_the_weights_sum_to_one_within_2_ulp():
    t = np.concatenate([np.arange(0.0, 1.0, 1.0 / 128.0), np.random.default_rng(0).random(300)]).astype(f32)
    assert (t >= 0).all() and (t < 1).all()
    k = TR.cubic_weights(t)
    exact = sum(x.astype(np.float64) for x in k)
    assert np.abs(exact - 1.0).max() <= 2.0 * 2.0 ** -23
    in_f32 = (((k[0] + k[1]).astype(f32) + k[2]).astype(f32) + k[3]).astype(f32)
    assert np.abs(in_f32.astype(np.float64) - 1.0).max() <= 2.0 * 2.0 ** -23
    assert all(float(x[0]) == v for x, v in zip(k, (0.0, 1.0, 0.0, 0.0)))  # t = 0


def test_the_anti_ringing_clamp_is_active_on_a_step_edge():
    """A history that is 0 left of column 4 and 1 from it on, resampled half a pixel aside: where the inner taps are both 1 and the outer
    left tap is 0, Catmull-Rom overshoots to 1.0625; the clamp brings it back into the inner range [1, 1]."""
    w, h = 8, 8
    pc, c, nr, rec, obj, prev, M = _ortho_case(w, h, 0.5, 0.0, 5, lengths=(2.0,))
    xs = np.tile(np.arange(w), h)
    prev[0][:, :3] = np.where(xs >= 4, f32(1.0), f32(0.0))[:, None]
    c[:] = f32(1.0)
    out, hist, _, arm, raw = TR.accumulate(w, h, c, nr, rec, obj, prev, None, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 1, want_unclamped=True)
    over = (arm == TR.ARM_CUBIC) & (raw[:, 0] > f32(1.0))
    assert over.any() and np.allclose(raw[over, 0], 1.0625)
    assert (out[over] == f32(1.0)).all()  # h = 1 after the clamp: out = h + a * (c - h) = 1 exactly
    under = (arm == TR.ARM_CUBIC) & (raw[:, 0] < f32(0.0))
    assert under.any() and (out[under, 0] == f32(1.0 / 3.0)).all()  # h clamped to 0, n' = 3: 0 + (1 / 3) * (1 - 0)


def test_non_finite_history_inside_a_full_footprint():
    """The constructed case of temporal_resample_cases.non_finite_history_case: footprints that are whole and hold a non-finite colour
    or moment.  The clamp returns a NaN or -inf h to the inner taps' range; where h stays +inf (the single inf as one of the four inner
    taps: 4 pixels; the block as all four: 1) the blend is NaN and step 5 resets the pixel; a non-finite moment falls back to (y, y2)
    while the colour keeps its blend."""
    w, h = 12, 10
    pc, c, nr, rec, obj, prev, M, clean_A, clean_M = K.non_finite_history_case(w, h)
    out, hist, mom, arm, raw = TR.accumulate(w, h, c, nr, rec, obj, prev, M, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 1, want_unclamped=True)
    clean = TR.accumulate(w, h, c, nr, rec, obj, (clean_A,) + prev[1:], clean_M, pc, 0.0, 0.0, [], 8, 0.05, -1.0, 1)
    was_cubic = clean[3] == TR.ARM_CUBIC
    assert was_cubic.sum() == (w - 3) * (h - 3)
    healed = (arm == TR.ARM_CUBIC) & ~np.isfinite(raw).all(axis=1)
    assert healed.sum() >= 12 + 16 + 8 and np.isnan(raw[healed]).any() and np.isinf(raw[healed]).any()  # the inf's ring, the NaN's 16, most of the block's
    assert np.isfinite(out).all() and np.isfinite(hist[0]).all()
    gone = was_cubic & (arm == TR.ARM_RESET)
    assert gone.sum() == 4 + 1 and bits_equal(out[gone], c[gone]) and (hist[0][gone, 3] == f32(1.0)).all()
    y = TV.luminance(c)
    fell = (arm == TR.ARM_CUBIC) & (mom[:, 0] == y) & (mom[:, 1] == (y * y).astype(f32))
    assert fell.any() and not bits_equal(out[fell], c[fell])  # the moments fell back, the colour blended
    assert np.isfinite(mom).all()


def test_the_rust_link_attribute_sits_on_the_extern_block():
    rs = open(os.path.join(ROOT, "bindings", "rayn_hip.rs")).read()
    assert rs.count("#[link(") == 1 and re.search(r'#\[link\(name = "rayn_hip"\)\]\nextern "C" \{', rs)


def test_temporal_resample_validation():
    import rayn_amd as R
    from rayn_amd import _abi
    assert R.Temporal().resample == "bilinear" and R.Temporal(resample="catmull_rom").resample_to_abi().resample == 1
    assert R.Temporal().resample_to_abi().resample == 0 and _abi.TEMPORAL_RESAMPLE == {"bilinear": 0, "catmull_rom": 1}
    for bad in ("nearest", "", 1, None, b"bilinear"):
        with pytest.raises(ValueError, match="resample"):
            R.Temporal(resample=bad)
    # the option travels in its own struct: rayn_temporal_params and the positional order of the older fields are what they were
    t = R.Temporal(8, 0.1, 0.5, 0.25, "catmull_rom")
    assert (t.max_history, t.depth_tolerance, t.normal_min, t.feedback, t.resample) == (8, 0.1, 0.5, 0.25, "catmull_rom")
    assert [f[0] for f in _abi.TemporalParams._fields_] == ["max_history", "depth_tolerance", "normal_min"]


def test_the_abi_struct_matches_the_compiled_library_and_the_mirrors():
    from rayn_amd import _abi, _lib
    _lib.build()
    L = _lib.lib()
    S = _abi.TemporalResampleParams
    assert C.sizeof(S) == L.rayn_hip_sizeof(7) == 4 and S.resample.offset == 0 and S.resample.size == 4
    assert hasattr(L, "rayn_hip_temporal_accumulate_resample_device")
    hdr = open(os.path.join(ROOT, "include", "rayn_hip.h")).read()
    assert re.search(r"typedef struct \{\s*uint32_t resample;[^}]*\}\s*rayn_temporal_resample_params;", hdr)
    rs = open(os.path.join(ROOT, "bindings", "rayn_hip.rs")).read()
    assert re.search(r"pub struct RaynTemporalResampleParams \{\s*pub resample: u32,\s*\}", rs)
    assert re.search(r"pub struct RaynTemporalParams \{\s*pub max_history: u32,\s*pub depth_tolerance: f32,\s*pub normal_min: f32,\s*\}", rs)
    assert "rayn_hip_temporal_accumulate_resample_device" in open(os.path.join(ROOT, "include", "rayn_host.hpp")).read()
