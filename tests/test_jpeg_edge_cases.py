"""The edge cases of the device JPEG encoder (tests/jpeg_edge_cases.py) held to account without a GPU: every claim, the kill matrix of
jpeg_np's mutants, the independent reader (tests/jpeg_read.py) on every file, Pillow's load of every file, libjpeg's reconstruction of the
image-level cases, and the reader itself on files it must refuse.  No GPU."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_cases as K
import jpeg_edge_cases as E
import jpeg_np as J
import jpeg_read as R
from jpeg_decode import CHROMA_BOUND, PLANE_BOUND, reconstruction_differences as _reconstruction_differences


def test_every_case_reaches_what_it_is_for():
    cases = E.cases()   # asserts every claim
    assert len(cases) == len(E.NAMES) >= 40 and set(E.IMAGE_NAMES) | set(E.COEF_NAMES) == set(E.NAMES)
    families = {c.name.split("/")[0] for c in cases}
    assert families == {"ac_size_10", "tie_signs", "colour_halves", "box_remainders", "zrl_ladder", "category_edges", "bit_phases", "pad_edges", "ff_runs",
                        "predictor_420", "one_byte_segments", "segment_counts", "scan_residues", "stale_buffers"}
    assert {int(c.name.split("/")[1]) for c in cases if c.name.startswith("segment_counts/")} == {8, 9, 16, 17, 256, 512, 513}
    assert max(c.ref.blocks for c in cases) <= 4000   # the smallest that reach the edge
    for c in cases:
        if c.kind == "coef":  # what rayn_hip_probe_jpeg_entropy accepts
            assert -1024 <= c.coef[:, 0].min() and c.coef[:, 0].max() <= 1023 and np.abs(c.coef[:, 1:]).max() <= 1023, c.name


def test_every_mutant_is_killed_by_a_case_that_names_it():
    kills = E.kill_matrix()
    assert sorted(kills) == sorted(J.MUTANTS) and set(E.NEW_MUTANTS) | set(E.OLD_MUTANTS) == set(J.MUTANTS) and len(E.OLD_MUTANTS) == 6
    for c in E.cases():
        for m in c.kills:
            assert c.name in kills[m], f"{c.name} names {m} and does not tell it from the definition"
    for m in J.MUTANTS:
        assert [c.name for c in E.cases() if m in c.kills], f"no case names the mutant {m}"
    # the cases made for a mutant, by name
    made_for = {"zrl_at_most_two": "zrl_ladder/grey_ri65535", "tie_positive_toward_zero": "tie_signs/q100", "ties_toward_zero_above_q1": "tie_signs/q95",
                "chroma_offset_32768": "colour_halves", "luma_truncates": "colour_halves", "box_truncates": "box_remainders/16x16", "pad_unstuffed": "pad_edges",
                "stuff_one_per_word": "ff_runs/two_words_per_thread", "y_pred_from_y00": "predictor_420", "first_mcu_resets_every_y": "predictor_420",
                "cbcr_share_predictor": "predictor_420"}
    assert sorted(made_for) == sorted(E.NEW_MUTANTS)
    for m, name in made_for.items():
        assert m in E.case(name).kills
    # a tie at Q = 1 does not tell "ties toward zero above Q = 1" from the definition, and the flat one-byte segments tell no arithmetic at all
    assert "tie_signs/q100" not in kills["ties_toward_zero_above_q1"]
    assert all(not n.startswith("one_byte_segments") for m in ("row_truncates", "ties_toward_zero", "luma_truncates") for n in kills[m])


def test_the_older_cases_still_kill_the_older_mutants():
    kills = K.mutant_kills()
    assert set(E.OLD_MUTANTS) <= set(kills)
    for m in E.OLD_MUTANTS:
        assert kills[m], m


@pytest.mark.parametrize("name", E.NAMES)
def test_the_reader_returns_the_coefficients_that_went_in(name):
    c = E.case(name)
    r = R.read(c.ref.file)
    assert r["coef"].shape == c.ref.coef.shape and np.array_equal(r["coef"], c.ref.coef), name
    assert np.array_equal(r["comp"], c.ref.block_comp) and (r["width"], r["height"], r["ri"]) == (c.width, c.height, c.ri)
    assert r["intervals"] == c.ref.segments and r["pad_bits"] == [-n % 8 for n in c.ref.segment_bits]
    if c.kind == "coef":
        assert np.array_equal(r["coef"], c.coef)


def test_the_reader_reads_the_older_cases_too():
    for name, c in K.cases().items():
        assert np.array_equal(R.read(c.ref.file)["coef"], c.ref.coef), name


@pytest.mark.parametrize("name", E.NAMES)
def test_pillow_loads_every_file_completely(name):
    c = E.case(name)
    im = Image.open(io.BytesIO(c.ref.file))
    im.load()
    assert im.size == (c.width, c.height) and im.mode == ("L" if c.bpp == 1 else "RGB")


@pytest.mark.parametrize("name", E.IMAGE_NAMES)
def test_libjpeg_reconstructs_what_the_coefficients_of_an_image_case_say(name):
    full, chroma = _reconstruction_differences(E.case(name))
    print(name, "full-resolution planes:", [int(v) for v in full], "4:2:0 chroma:", chroma)
    assert max(full) <= PLANE_BOUND, (name, full)
    assert max(chroma, default=0.0) <= CHROMA_BOUND, (name, chroma)


def test_the_reader_tells_the_mutants_of_the_entropy_layer_apart():
    """The reader is no echo of the restatement: on the scans of the mutants that break the format (not merely choose other coefficients)
    it raises or returns other coefficients"""
    for name, mutants in (("pad_edges", ("pad_zero", "pad_unstuffed")), ("ff_runs/three_in_a_row", ("stuff_one_per_word",)), ("segment_counts/17", ("marker_unwrapped",)),
                          ("zrl_ladder/grey_ri1", ("zrl_at_most_two", "eob_always")), ("predictor_420", ("y_pred_from_y00", "first_mcu_resets_every_y", "cbcr_share_predictor", "predictor_kept"))):
        c = E.case(name)
        for m in mutants:
            data = J.frame(c.width, c.height, c.bpp, 100, c.subsampling, c.ri, c.mutant(m).scan)
            try:
                same = np.array_equal(R.read(data)["coef"], c.ref.coef)
            except (ValueError, IndexError):
                same = False
            assert not same, (name, m)


def test_the_reader_refuses_what_is_not_a_baseline_file():
    c = E.case("segment_counts/9")
    good = c.ref.file
    assert R.read(good)["intervals"] == 9
    sos = good.index(b"\xff\xda")
    for bad, text in ((good[:-2], "no EOI"), (good + b"\0", "behind EOI"), (b"\0" + good, "no SOI"), (good.replace(b"\xff\xd1", b"\xff\xd2", 1), "out of order"),
                      (good.replace(b"\xff\xc0", b"\xff\xc2", 1), "not a baseline"), (good[:sos + 4 + 3] + b"\x01" + good[sos + 4 + 4:], "Ss, Se")):
        with pytest.raises(ValueError, match=text):
            R.read(bad)


def test_entropy_is_the_second_half_of_encode():
    """jpeg_np.entropy on the coefficients of jpeg_np.coefficients is jpeg_np.encode, mutants of either half included"""
    c = K.cases()["size_17x33_420"]
    for m in (None, "cbcr_share_predictor", "box_truncates"):
        whole = J.encode(c.img, c.quality, c.subsampling, c.ri, m)
        first = J.coefficients(c.img, c.quality, c.subsampling, m)
        assert J.entropy(first.coef, first.block_comp, 3, c.subsampling, c.ri, m).scan == whole.scan
    assert J.encode(c.img, c.quality, c.subsampling, c.ri, "cbcr_share_predictor").scan != c.ref.scan
