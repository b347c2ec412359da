"""The preview integrator on the CPU: the numpy restatement (tests/preview_np.py) against the oracle and against geometry whose answer is
known, the coverage conditions of every GPU case, the sampling maps on the tables the cases use, Preview's validation, the scratch size and
the render_sequence argument combinations that must raise.  No GPU."""
import inspect

import numpy as np
import pytest

import preview_np as PN
import restatement_np as RN
import temporal_np as T
from common import bits_equal

f32 = np.float32


def test_primary_hits_are_the_oracles_closest_hit_at_the_pixel_centres(oracle):
    """records and objects of the restatement = oracle closest_hit at depth 0 on the pixel-centre rays of the world frozen at time_start,
    for a static and a moving case; background pixels carry colour 0, alpha 0, normal 0 and ao 1."""
    for case in (PN.CASES[2], PN.CASES[10]):
        wd, p, _, _ = PN.case_inputs(case)
        ref = PN.case_reference(oracle, case)
        org, dirs = T.pixel_centre_rays(oracle, wd, p)
        t, obj = oracle.closest_hit(T.frozen_world(wd, p.time_start), p, 0, org, dirs)
        assert np.array_equal(ref["object"], obj) and bits_equal(ref["records"][:, 3], t)
        with np.errstate(all="ignore"):
            assert bits_equal(ref["records"][:, :3], (org + (t[:, None] * dirs).astype(f32)).astype(f32))
        bg = ~ref["surface"]
        assert bg.any() and not ref["color"][bg].any() and not ref["alpha"][bg].any() and not ref["normal"][bg].any() and np.all(ref["ao"][bg] == 1.0)
        assert np.all(ref["alpha"][~bg] == 1.0)
        sky = np.array([wd.materials[wd.hitables[int(o)].material].kind == PN.MAT_SKY for o in obj])
        assert np.array_equal(bg, sky)  # under the dome every centre ray hits something: the background is the sky


def _two_spheres(res, second):
    """The sky dome, a unit sphere at the origin and, when asked, a second one resting against it beside it as the camera sees them"""
    import rayn_amd as A
    from rayn_amd import setup as S
    from rayn_amd.scene import Sphere
    cam, world = S.setup_s0(res)
    grey = world.hitables[1].material
    del world.hitables[1:]
    world.lights = []
    world.hitables.push(Sphere(A.vec3(0.0, 0.0, 0.0), 1.0, grey))
    if second:
        c = np.array([2.0, 0.0, 0.45])  # at right angles to the camera's axis (-0.45, 0.2, 2.0): the contact is in view on both spheres
        c = c / np.sqrt(c @ c) * 1.5  # touching: centre distance 1.5 = 1.0 + 0.5
        world.hitables.push(Sphere(A.vec3(*c), 0.5, grey))
    return world.to_desc(cam)


def test_a_free_hemisphere_has_ao_one_and_a_resting_sphere_shadows(oracle):
    """Spheres only.  Alone, a convex sphere's hemisphere of any radius is free: ao = 1 on every surface pixel, and the colour is the
    headlight term alone.  With a second sphere resting against it, the pixels around the contact have ao < 1 on both spheres, the normals
    are unit and face the viewer, and 0 <= ao <= 1 everywhere."""
    import rayn_amd as A
    from rayn_amd import film as F
    w, h, K = 40, 24, 8
    p = A.frame_params(w, h, 1, 0)
    samples, scramble = F.preview_tables(K, 1, w, h)
    alone = PN.preview(oracle, _two_spheres((w, h), False), p, samples, scramble, 0.75, 0.3)
    s = alone["surface"]
    assert 20 < s.sum() < w * h and np.all(alone["ao"][s] == 1.0) and set(alone["object"][s].tolist()) == {1}
    nf = alone["normal"][s].astype(np.float64)
    assert np.allclose((nf * nf).sum(1), 1.0, atol=1e-6)
    _, dirs = T.pixel_centre_rays(oracle, _two_spheres((w, h), False), p)
    ndv = -(nf * dirs[s].astype(np.float64)).sum(1)
    assert np.all(ndv > 0.0)
    assert np.allclose(alone["color"][s, 0], 0.3 + 0.7 * ndv, atol=1e-6) and np.array_equal(alone["color"][:, 0], alone["color"][:, 2])
    both = PN.preview(oracle, _two_spheres((w, h), True), p, samples, scramble, 0.75, 0.3)
    on_big, on_small = both["object"] == 1, both["object"] == 2
    assert on_big.sum() > 10 and on_small.sum() > 10
    assert (both["ao"][on_big] < 1.0).any() and (both["ao"][on_small] < 1.0).any()
    assert np.all((both["ao"] >= 0.0) & (both["ao"] <= 1.0)) and np.all(both["ao"] * K == np.round(both["ao"] * K))
    assert both["sphere_stop"].any() and not both["sdf_stop"].any()


@pytest.mark.parametrize("case", PN.CASES, ids=[c[0] for c in PN.CASES])
def test_cases_meet_the_coverage_conditions_and_the_sampling_maps_agree(oracle, case):
    """Every GPU case on the restatement alone: the coverage conditions hold (the spheres-only scene has no TracedSDF, so the two about SDF
    scenes do not apply), and on the very (u, v) pairs and normals the case uses, the oracle's own cosine_weighted_in_hemisphere and
    get_orthonormal_basis (probe_shading ops 2 and 4) give the bits of the numpy functions the restatement calls - the binary64 sine and
    cosine rounded once, which could differ from the pinned ones on a near-tie, do not on these tables."""
    ref = PN.case_reference(oracle, case)
    PN.check_coverage(ref, case[1] != "spheres")
    wd, _, samples, scramble = PN.case_inputs(case)
    sel = np.flatnonzero(ref["surface"])
    uv = PN.ao_inputs(samples, scramble, sel)
    assert uv.shape == (len(sel) * case[5], 2) and np.all((uv >= 0.0) & (uv < 1.0))
    fma = bool(case[6])
    nf = ref["normal"][sel]
    with RN.fused_policy(fma), np.errstate(all="ignore"):
        l = np.stack(RN.cosine_weighted_in_hemisphere(uv[:, 0].copy(), uv[:, 1].copy()), axis=1).astype(f32)
        b = np.stack([c for col in RN.onb([nf[:, 0].copy(), nf[:, 1].copy(), nf[:, 2].copy()]) for c in col], axis=1).astype(f32)
    assert bits_equal(oracle.probe_shading(wd, 2, 0, uv, fma=fma), l)
    assert bits_equal(oracle.probe_shading(wd, 4, 0, nf, fma=fma), b)


def test_preview_validation():
    import rayn_amd as R
    assert R.Preview() == R.Preview(8, 0.4, 0.3) and R.Preview(64, 1e-3, 0.0).to_abi().samples == 64 and R.Preview(1, 5, 1).to_abi().ambient == 1.0
    for kw, text in ((dict(samples=0), "samples"), (dict(samples=65), "samples"), (dict(samples=4.0), "samples"), (dict(samples=True), "samples"),
                     (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"), (dict(radius=float("inf")), "radius"), (dict(radius=float("nan")), "radius"),
                     (dict(radius=1e-60), "radius"), (dict(radius=1e60), "radius"), (dict(radius="1"), "radius"), (dict(ambient=-0.1), "ambient"),
                     (dict(ambient=1.5), "ambient"), (dict(ambient=float("nan")), "ambient"), (dict(ambient=None), "ambient")):
        with pytest.raises(ValueError, match=f"Preview.{text}"):
            R.Preview(**kw)


def test_preview_scratch_bytes():
    """0 for a size the entry rejects and for samples outside 1..64; otherwise the documented count, monotone in every argument."""
    from rayn_amd import film as F
    sb = F.preview_scratch_bytes
    for w, h, k in ((0, 8, 4), (8, 0, 4), (65536, 32768, 4), (8, 8, 0), (8, 8, 65)):
        assert sb(w, h, k) == 0, (w, h, k)
    assert sb(46340, 46340, 64) > 0  # just under 2^31 pixels
    for w, h in ((1, 1), (37, 23), (64, 40), (1280, 720)):
        npad = (w * h + 63) // 64 * 64
        for k in (1, 4, 8, 9, 64):
            assert sb(w, h, k) == F.gbuffer_scratch_bytes(w, h) + 32 * npad + 29 * min(k, 8) * npad, (w, h, k)
    sizes = [(1, 1), (8, 8), (9, 8), (37, 23), (64, 40), (65, 40), (1280, 720), (1920, 1080)]
    for k in (1, 8, 64):
        got = [sb(w, h, k) for w, h in sizes]
        assert got == sorted(got) and got[0] > 0
    for w, h in sizes:
        got = [sb(w, h, k) for k in range(1, 65)]
        assert got == sorted(got)


def test_render_sequence_argument_combinations_that_must_raise(tmp_path):
    import rayn_amd as R
    from rayn_amd import film as F
    K = R.ChannelKind
    C, A, B, N = K.Color, K.Alpha, K.Background, K.WorldNormal
    K4, pv = [C, A, B, N], R.Preview()
    for kinds, write, options, text in (
            (K4, [C], dict(preview=4), "preview must be a Preview, got 4"),
            (K4, [C], dict(preview=pv, upscale=R.Upscale(2)), "preview= with upscale= or supersample= is not built"),
            (K4, [C], dict(preview=pv, upscale=R.Upscale(2), temporal=R.Temporal(), supersample=R.Supersample()), "preview= with upscale= or supersample= is not built"),
            (K4, [C], dict(preview=pv, supersample=R.Supersample()), "preview= with upscale= or supersample= is not built"),
            (K4, [C], dict(preview=pv, denoise=R.VarianceDenoise()), "preview= with a VarianceDenoise is not built"),
            (K4, [C], dict(preview=pv, denoise=R.VarianceDenoise(), temporal=R.Temporal()), "preview= with a VarianceDenoise is not built"),
            ([A, N], [A], dict(preview=pv), "Attempted to preview into a film without a Color channel"),
            ([C, A], [C], dict(preview=pv, temporal=R.Temporal()), "temporal accumulation needs the film's Color and WorldNormal channels"),
            ([C, A], [C, B], dict(preview=pv), "Attempted to write Background channel but it didn't exist")):
        with pytest.raises(ValueError) as e:
            F.plan_sequence(kinds, write, False, **options)
        assert text in str(e.value), (options, str(e.value))
    # what composes, and the names
    plan = F.plan_sequence(K4, [C, A, N], preview=pv, denoise=R.Denoise(), display=R.Display(), temporal=R.Temporal())
    assert [s for _, _, s in plan.jobs] == ["color_preview_temporal_denoised_display", "alpha", "normal"] and plan.preview is pv
    assert [s for _, _, s in F.plan_sequence([C], [C], preview=pv).jobs] == ["color_preview"]
    assert F.plan_sequence(K4, [C]).preview is None
    sig = inspect.signature(R.Film.render_sequence)
    assert sig.parameters["preview"].default is None
    # render_sequence raises the plan's error before it touches anything
    film = R.Film.__new__(R.Film)
    film._init_state(K4, (24, 16), None, "cuda:0")
    with pytest.raises(ValueError, match="preview= with upscale="):
        film.render_sequence(None, None, None, None, (16, 16), [1], 24, 1.0 / 24.0, 1, [C], str(tmp_path / "no"), "a", preview=pv, upscale=R.Upscale(2))
    assert not (tmp_path / "no").exists()
    with pytest.raises(ValueError, match="preview must be a Preview"):
        film.render_preview(preview=3)
