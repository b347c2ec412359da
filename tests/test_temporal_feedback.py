"""The feedback of the filtered colour into the temporal history, without a GPU: the validation of Temporal(feedback=), the argument rule of
Film.render_sequence, and properties of the numpy restatement of the write-back (tests/temporal_feedback_np.py) on an adversarial history
and film.  tests/test_temporal_feedback_device.py holds the kernels to the restatement bit for bit."""
import os

import numpy as np
import pytest

import temporal_feedback_np as TF
import temporal_np as T
import temporal_variance_np as TV
from temporal_feedback_cases import H0, SIGMAS, W0, adversarial_inputs, restate

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- the parameter ------------------------------------------------------------------------------------------------------------------------

def test_temporal_feedback_is_validated_like_its_neighbours():
    import rayn_amd as R
    assert R.Temporal().feedback == 0.0
    for ok in (0, 0.0, 0.25, 1, 1.0, np.float32(0.5), np.int32(1)):
        assert float(R.Temporal(feedback=ok).feedback) == float(ok)
    for bad in (float("nan"), float("inf"), -float("inf"), -0.25, 1.0000001, 2, -1):
        with pytest.raises(ValueError, match="Temporal.feedback must be finite and in"):
            R.Temporal(feedback=bad)
    for bad in (True, "0.5", None, [0.5]):
        with pytest.raises(ValueError, match="Temporal.feedback must be a number"):
            R.Temporal(feedback=bad)
    # the strength travels as the entry's argument: rayn_temporal_params and the positional order of the other fields are what they were
    t = R.Temporal(8, 0.25, 0.5, 0.75)
    assert (t.max_history, t.depth_tolerance, t.normal_min, t.feedback) == (8, 0.25, 0.5, 0.75)
    abi = t.to_abi()
    assert [f[0] for f in abi._fields_] == ["max_history", "depth_tolerance", "normal_min"]
    assert (abi.max_history, abi.depth_tolerance, abi.normal_min) == (8, 0.25, 0.5)


def test_render_sequence_with_feedback_and_no_variance_denoiser_raises_before_anything_runs(tmp_path):
    """The film is never rendered (there may be no GPU): the argument check comes first and nothing is written."""
    import rayn_amd as R
    K = R.ChannelKind
    film = R.Film.__new__(R.Film)  # no context: the check must not need one
    for denoise in (None, R.Denoise()):
        with pytest.raises(ValueError, match="Temporal.feedback > 0 feeds a VarianceDenoise's first pass back"):
            film.render_sequence(None, None, None, None, (16, 16), [1], 24, 1.0 / 24.0, 1, [K.Color], str(tmp_path / "seq"), "a", denoise=denoise,
                                 temporal=R.Temporal(feedback=0.5))
    assert not os.path.exists(tmp_path / "seq")


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def case(oracle):
    """One adversarial input and the restatement's result for every combination of terms at beta = 0, 0.5 and 1; computed once, not modified."""
    inp = adversarial_inputs(W0, H0, 11)
    res = {(s, beta): restate(W0, H0, inp, 1, s, beta) for s in SIGMAS for beta in (0.0, 0.5, 1.0)}
    return inp, res


def test_the_case_has_substance(case):
    inp, res = case
    n = W0 * H0
    A = T.split_history(inp["hist"], n)[0]
    v0, _ = TV.initial_variance(W0, H0, inp["color"], inp["obj"], A[:, 3], inp["mom"])
    guided = ~np.isnan(v0)
    assert guided.sum() > 200 and (~guided).sum() > 100
    assert not np.isfinite(A[:, :3]).all() and (A[:, :3] == 3.0e38).any()
    for s in SIGMAS:
        _, v1, (A1, _, _, _) = res[(s, 1.0)]
        changed = (_bits(A1[:, :3]) != _bits(A[:, :3])).any(axis=1)
        assert changed.sum() > 200, s
        # a guided pixel whose blend is not finite keeps its history; the luminance term gives a tap that far away no weight, so the
        # combinations with it cannot get there.  (Pass 0's overflow rule needs a sum of weighted colours to round past the largest
        # float; these inputs do not reach it, and a pixel it drops has v' = NaN like one that was never guided.)
        c1, v1 = TF.first_pass(W0, H0, inp["color"], inp["alpha"], inp["normal"], inp["obj"], A[:, 3], inp["mom"], *s)
        with np.errstate(all="ignore"):
            fb = (inp["color"] + (f32(0.5) * (c1 - inp["color"]).astype(f32)).astype(f32)).astype(f32)
        assert (~np.isnan(v1) & ~np.isfinite(fb).all(axis=1)).any() == (s[0] == 0.0), s


def test_a_strength_of_zero_leaves_every_bit_of_the_history(case):
    inp, res = case
    hist = T.split_history(inp["hist"], W0 * H0)
    for s in SIGMAS:
        for a, b in zip(res[(s, 0.0)][2], hist):
            assert np.array_equal(_bits(a), _bits(b)), s


def test_only_the_colour_of_plane_a_is_ever_written(case):
    inp, res = case
    A, B, N, O = T.split_history(inp["hist"], W0 * H0)
    for key, (_, _, (A1, B1, N1, O1)) in res.items():
        assert np.array_equal(_bits(A1[:, 3]), _bits(A[:, 3])), key  # n' keeps its bits, a NaN's payload included
        assert np.array_equal(_bits(B1), _bits(B)) and np.array_equal(_bits(N1), _bits(N)) and np.array_equal(O1, O), key


def test_a_pixel_with_a_history_keeps_a_finite_colour(case):
    inp, res = case
    for key, (_, _, (A1, _, _, _)) in res.items():
        with np.errstate(invalid="ignore"):
            has_history = A1[:, 3] >= f32(1.0)
        assert has_history.sum() > 500 and np.isfinite(A1[has_history, :3]).all(), key


def test_pixels_that_are_not_guided_are_untouched_and_the_outputs_do_not_depend_on_the_strength(case):
    inp, res = case
    n = W0 * H0
    A = T.split_history(inp["hist"], n)[0]
    v0, _ = TV.initial_variance(W0, H0, inp["color"], inp["obj"], A[:, 3], inp["mom"])
    not_guided = np.isnan(v0)
    for (s, beta), (c, v, (A1, _, _, _)) in res.items():
        assert np.array_equal(_bits(A1[not_guided]), _bits(A[not_guided])), (s, beta)
        c0, v0_, _ = res[(s, 0.0)]
        assert np.array_equal(_bits(c), _bits(c0)) and np.array_equal(_bits(v), _bits(v0_)), (s, beta)


def test_a_strength_of_one_writes_the_first_pass_up_to_one_rounding_and_a_half_lies_between(case):
    """fb = c + 1 * (c' - c) is c' up to the rounding of the subtraction and the addition; at 0.5 it lies between c and c'."""
    inp, res = case
    n = W0 * H0
    A = T.split_history(inp["hist"], n)[0]
    s = (4.0, 0.4, 0.3)
    c = inp["color"].astype(np.float64)
    c1, v1 = TF.first_pass(W0, H0, inp["color"], inp["alpha"], inp["normal"], inp["obj"], A[:, 3], inp["mom"], *s)
    for beta in (0.5, 1.0):
        A1 = res[(s, beta)][2][0]
        written = (_bits(A1[:, :3]) != _bits(A[:, :3])).any(axis=1)
        assert written.sum() > 200 and not np.isnan(v1[written]).any()
        lo, hi = np.minimum(c, c1)[written], np.maximum(c, c1)[written]
        with np.errstate(over="ignore"):  # the spacing at the largest float
            slack = 4.0 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(f32)).astype(np.float64)
        got = A1[written, :3].astype(np.float64)
        assert np.all(got >= lo - slack) and np.all(got <= hi + slack), beta
        if beta == 1.0:
            assert np.all(np.abs(got - c1[written]) <= slack)
