"""plan_sequence: what a render_sequence call runs and what its files are called, decided on the host before anything renders.
The suffixes are those of render_sequence's docstring, as literals."""
import pytest

import rayn_amd as R
from rayn_amd import film as F

K = R.ChannelKind
C, A, B, N = K.Color, K.Alpha, K.Background, K.WorldNormal
K4, K2, KCN = [C, A, B, N], [C, A], [C, N]
DEN, VAR, TMP, DSP, UP, SUP = R.Denoise(), R.VarianceDenoise(), R.Temporal(), R.Display(), R.Upscale(2), R.Supersample()
OPTIONS = ("denoise", "display", "upscale", "supersample", "temporal")

# (id, kinds, write_channels, transparent_background, options, {kind: (suffix, bpp)}, options that come back None)
ROWS = [
    ("plain", K4, K4, False, {}, {C: ("color", 3), A: ("alpha", 1), B: ("background", 3), N: ("normal", 3)}, OPTIONS),
    ("plain-transparent", K4, [C, A], True, {}, {C: ("color", 4), A: ("alpha", 1)}, OPTIONS),
    ("denoise", K4, K4, False, dict(denoise=DEN), {C: ("color_denoised", 3), A: ("alpha", 1), B: ("background", 3), N: ("normal", 3)},
     ("display", "upscale", "supersample", "temporal")),
    ("temporal", K4, [A, N, C], False, dict(temporal=TMP), {A: ("alpha", 1), N: ("normal", 3), C: ("color_temporal", 3)},
     ("denoise", "display", "upscale", "supersample")),
    ("temporal-variance", K4, [C], False, dict(denoise=VAR, temporal=TMP), {C: ("color_temporal_denoised", 3)}, ("display", "upscale", "supersample")),
    ("temporal-denoise", K4, [C], True, dict(denoise=DEN, temporal=TMP), {C: ("color_temporal_denoised", 4)}, ("display", "upscale", "supersample")),
    ("display", K4, [C, A], False, dict(display=DSP), {C: ("color_display", 3), A: ("alpha", 1)}, ("denoise", "upscale", "supersample", "temporal")),
    ("upscale", K4, K4, False, dict(upscale=UP), {C: ("color_x2", 3), A: ("alpha_x2", 1), B: ("background_x2", 3), N: ("normal_x2", 3)},
     ("denoise", "display", "supersample", "temporal")),
    ("upscale-transparent", K4, [C], True, dict(upscale=R.Upscale(3)), {C: ("color_x3", 4)}, ("denoise", "display", "supersample", "temporal")),
    ("supersample", K4, [C, A], False, dict(upscale=UP, temporal=TMP, supersample=SUP), {C: ("color_temporal_x2", 3), A: ("alpha_x2", 1)},
     ("denoise", "display")),
    ("denoise-display-upscale", K4, [C], False, dict(denoise=DEN, display=DSP, upscale=UP), {C: ("color_denoised_display_x2", 3)},
     ("supersample", "temporal")),
    ("all-one-size", K4, K4, False, dict(denoise=VAR, temporal=TMP, display=DSP),
     {C: ("color_temporal_denoised_display", 3), A: ("alpha", 1), B: ("background", 3), N: ("normal", 3)}, ("upscale", "supersample")),
    ("all", K4, K4, False, dict(denoise=DEN, temporal=TMP, display=DSP, upscale=UP, supersample=SUP),
     {C: ("color_temporal_denoised_display_x2", 3), A: ("alpha_x2", 1), B: ("background_x2", 3), N: ("normal_x2", 3)}, ()),
    ("all-transparent", K4, [C, A], True, dict(denoise=DEN, temporal=TMP, display=DSP, upscale=UP, supersample=SUP),
     {C: ("color_temporal_denoised_display_x2", 4), A: ("alpha_x2", 1)}, ()),
    # nothing writes Color: temporal, display, denoise and supersample switch themselves off and the plain suffixes stay
    ("no-color-all-one-size", K4, [A, N], False, dict(denoise=VAR, temporal=TMP, display=DSP), {A: ("alpha", 1), N: ("normal", 3)}, OPTIONS),
    ("no-color-denoise", K4, [A, B], True, dict(denoise=DEN, display=DSP), {A: ("alpha", 1), B: ("background", 3)}, OPTIONS),
    ("no-color-all", K4, [A, N], False, dict(denoise=DEN, temporal=TMP, display=DSP, upscale=UP, supersample=SUP),
     {A: ("alpha_x2", 1), N: ("normal_x2", 3)}, ("denoise", "display", "supersample", "temporal")),
    # a [Color, Alpha] film
    ("two-plain", K2, K2, False, {}, {C: ("color", 3), A: ("alpha", 1)}, OPTIONS),
    ("two-transparent", K2, K2, True, {}, {C: ("color", 4), A: ("alpha", 1)}, OPTIONS),
    ("two-denoise-display", K2, K2, False, dict(denoise=DEN, display=DSP), {C: ("color_denoised_display", 3), A: ("alpha", 1)},
     ("upscale", "supersample", "temporal")),
    ("two-upscale", K2, K2, True, dict(upscale=UP), {C: ("color_x2", 4), A: ("alpha_x2", 1)}, ("denoise", "display", "supersample", "temporal")),
    ("two-no-color", K2, [A], False, dict(denoise=DEN, display=DSP, upscale=UP), {A: ("alpha_x2", 1)}, ("denoise", "display", "supersample", "temporal")),
]


@pytest.mark.parametrize("kinds,write,transparent,options,want,none", [r[1:] for r in ROWS], ids=[r[0] for r in ROWS])
def test_plan_table(kinds, write, transparent, options, want, none):
    plan = F.plan_sequence(kinds, write, transparent, **options)
    assert [(k, s, b) for k, b, s in plan.jobs] == [(k, *want[k]) for k in write]
    assert {o for o in OPTIONS if getattr(plan, o) is None} == set(none)
    for o in set(options) - set(none) - {"denoise", "upscale"}:
        assert getattr(plan, o) is options[o]
    assert plan.variance == isinstance(options.get("denoise"), R.VarianceDenoise)
    assert plan.transparent_background is transparent
    s = options["upscale"].factor if "upscale" in options else 1
    assert plan.out_res((24, 16)) == (24 * s, 16 * s)
    assert plan.up_keys == ([F._CHANNEL_KEY[k] for k in K if k in kinds] if "upscale" in options else None)


def test_guides_the_film_lacks_switch_their_sigma_off():
    assert F.plan_sequence(K4, [C], denoise=DEN).denoise == DEN
    assert F.plan_sequence(K2, [C], denoise=DEN).denoise == R.Denoise(sigma_normal=0.0)
    assert F.plan_sequence(KCN, [C], denoise=DEN).denoise == R.Denoise(sigma_alpha=0.0)
    assert F.plan_sequence([C], [C], denoise=DEN).denoise == R.Denoise(sigma_normal=0.0, sigma_alpha=0.0)
    up = R.Upscale(2, sigma_plane=0.1)
    assert F.plan_sequence(K4, [C], upscale=up).upscale == up
    plan = F.plan_sequence(K2, [C], upscale=up)
    assert plan.upscale == R.Upscale(2, sigma_plane=0.0) and plan.up_keys == ["color", "alpha"]
    # a VarianceDenoise's guides are required, not switched off
    assert F.plan_sequence(K4, [C], denoise=VAR, temporal=TMP).denoise is VAR
    no_alpha = R.VarianceDenoise(sigma_alpha=0.0)
    assert F.plan_sequence(KCN, [C], denoise=no_alpha, temporal=TMP).denoise is no_alpha


@pytest.mark.parametrize("kinds,write,options,text", [
    (K2, [C], dict(temporal=TMP), "temporal accumulation needs the film's Color and WorldNormal channels"),
    (K2, [A], dict(temporal=TMP), "temporal accumulation needs the film's Color and WorldNormal channels"),
    (K2, [C], dict(denoise=VAR, temporal=TMP), "temporal accumulation needs the film's Color and WorldNormal channels"),
    (KCN, [C], dict(denoise=VAR, temporal=TMP), "variance-guided denoising of a temporal sequence needs the film's Alpha channel when sigma_alpha != 0"),
    ([A, N], [A], dict(denoise=VAR, temporal=TMP), "Attempted to denoise the Color channel but it didn't exist"),
    ([A, N], [A], dict(upscale=UP), "Attempted to upscale a film without a Color channel"),
    (K2, [C, B], dict(display=DSP), "Attempted to write Background channel but it didn't exist"),
    ([C], [C], dict(denoise=DEN, display=4), "display must be a Display, got 4"),
    (K4, [C], dict(denoise=VAR), "render_sequence renders plain frames: VarianceDenoise needs the state of a progressive render"),
    (K4, [C], dict(temporal=R.Temporal(feedback=0.5)), "Temporal.feedback > 0 feeds a VarianceDenoise's first pass back into the history: pass one as `denoise`"),
    (K4, [C], dict(upscale=UP, temporal=TMP), "temporal= together with upscale= is not built: the temporal histories live at one resolution"),
    (K4, [C], dict(supersample=SUP, upscale=UP), "supersample= joins upscale= and temporal=: pass both"),
    # the first error raised wins: the combination before the channels, the channels before the options' own needs
    (K2, [B], dict(upscale=UP, temporal=TMP), "temporal= together with upscale= is not built: the temporal histories live at one resolution"),
    (K2, [B], dict(temporal=TMP), "Attempted to write Background channel but it didn't exist"),
])
def test_plan_errors(kinds, write, options, text):
    with pytest.raises(ValueError) as e:
        F.plan_sequence(kinds, write, False, **options)
    assert str(e.value) == text


def test_render_sequence_plans_before_it_touches_anything(tmp_path):
    """Film.render_sequence raises the plan's error with no context and creates no directory."""
    film = R.Film.__new__(R.Film)
    film._init_state(K2, (24, 16), None, "cuda:0")
    out = tmp_path / "no"
    with pytest.raises(ValueError, match="Attempted to write Background channel but it didn't exist"):
        film.render_sequence(None, None, None, None, (16, 16), [1], 24, 1.0 / 24.0, 1, [B], str(out), "anim")
    assert not out.exists()
