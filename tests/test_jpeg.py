"""The baseline JPEG definition of include/rayn_hip.h on the CPU: the restatement (tests/jpeg_np.py) on the named cases
(tests/jpeg_cases.py) against libjpeg through Pillow, the library's host-only exports against both, the framing of
rayn_amd.image.jpeg_from_scan, and rayn_amd.image.AviWriter against a reader written from the container's layout (tests/avi_read.py).
No GPU."""
import ctypes as C
import io
import os

import numpy as np
import pytest

from PIL import Image  # the decoder the files are pinned against: its absence is a failure, not a skip

import avi_read
import jpeg_cases as K
import jpeg_np as J
from jpeg_decode import CHROMA_BOUND, PLANE_BOUND, decode as _decode, reconstruction_differences as _reconstruction_differences


@pytest.fixture(scope="module")
def L():
    from rayn_amd import _lib
    _lib.build()
    return _lib.lib()


def test_every_case_reaches_what_it_is_for_and_every_mutant_is_killed():
    cases = K.cases()  # asserts every case's claim
    assert len(cases) == len(K.NAMES) >= 30
    kills = K.mutant_kills()
    assert sorted(kills) == sorted(K.MUTANTS) and K.MUTANTS == J.MUTANTS[:6]  # the later ones: tests/test_jpeg_edge_cases.py
    for m, names in kills.items():
        assert names, f"no case tells the mutant {m} from the definition"
    # each mutant falls to a case made for it
    assert "rounding_edges" in kills["row_truncates"] and "rounding_edges" in kills["ties_toward_zero"]
    assert "rst_wraps" in kills["marker_unwrapped"] and "checkerboard" in kills["eob_always"] and "padded_ff" in kills["pad_zero"]
    assert "dc_category_11" not in kills["predictor_kept"] and "ri_1" in kills["predictor_kept"]  # one segment keeps nothing


@pytest.mark.parametrize("name", K.NAMES)
def test_pillow_decodes_every_case(name):
    c = K.cases()[name]
    im = _decode(c.ref.file, False)
    assert im.size == (c.width, c.height) and im.mode == ("L" if c.bpp == 1 else "RGB")


@pytest.mark.parametrize("name", K.NAMES)
def test_libjpeg_reconstructs_what_the_coefficients_say(name):
    c = K.cases()[name]
    full, chroma = _reconstruction_differences(c)
    print(name, "full-resolution planes:", [int(v) for v in full], "4:2:0 chroma:", chroma)
    assert max(full) <= PLANE_BOUND, (name, full)
    assert max(chroma, default=0.0) <= CHROMA_BOUND, (name, chroma)


def test_library_quantisation_tables_are_libjpegs(L):
    img = Image.fromarray(K.cases()["size_17x33_444"].img)
    for q in (1, 10, 49, 50, 51, 90, 100):
        b = io.BytesIO()
        img.save(b, "JPEG", quality=q)
        pillow = Image.open(io.BytesIO(b.getvalue())).quantization  # {id: 64 entries, row-major}
        in_file = {seg[0]: list(seg[1:65]) for m, seg in J.segments_of(b.getvalue())[0] if m == 0xDB for seg in [seg[k:k + 65] for k in range(0, len(seg), 65)]}
        for which in (0, 1):
            out = (C.c_uint8 * 64)()
            assert L.rayn_jpeg_quant_table(q, which, out) == 0
            assert list(out) == in_file[which], (q, which)                                # zigzag, as the DQT segment holds it
            assert [out[k] for k in np.argsort(J.ZIGZAG)] == list(pillow[which]), (q, which)  # row-major, as Pillow reports it
            assert list(out) == [int(v) for v in J.quant_table(q, which)[J.ZIGZAG]]
    out = (C.c_uint8 * 64)()
    for q, which in ((0, 0), (101, 0), (50, 2)):
        assert L.rayn_jpeg_quant_table(q, which, out) == -1


def test_library_huffman_tables_are_libjpegs(L):
    for which in range(4):
        bits, vals = (C.c_uint8 * 16)(), (C.c_uint8 * 256)()
        n = L.rayn_jpeg_huffman_table(which, bits, vals, 256)
        want_bits, want_vals = J.tables()[1][(which & 1, which >> 1)]  # parsed from the DHT segments of a Pillow file
        assert n == len(want_vals) == (162 if which & 1 else 12)
        assert list(bits) == want_bits and list(vals[:n]) == want_vals
    assert L.rayn_jpeg_huffman_table(4, bits, vals, 256) == -1


def _bound_args(c):
    return c.width, c.height, c.bpp, c.subsampling, c.ri


def test_scan_bound_holds_on_every_case_and_is_within_a_factor_of_noise(L):
    for name, c in K.cases().items():
        bound = L.rayn_jpeg_scan_bound(*_bound_args(c))
        assert bound % 16 == 0 and bound >= 16 + len(c.ref.scan) + (-len(c.ref.scan) % 4), name
        assert L.rayn_jpeg_scratch_bytes(*_bound_args(c)) % 16 == 0
    # The bound charges every sample the longest code and 10 value bits, 26 bits, twice (the stuffing): 6.5 bytes a sample, the DC's few
    # bits more per block.  Uniform noise is incompressible, and at quality 100 (every Q = 1) the code is all but lossless, so its scan
    # cannot be shorter than the image's own bytes, 1 a sample (the case claims that much): the bound is reached within a factor of 7.
    c = K.cases()["noise_q100"]
    bound = L.rayn_jpeg_scan_bound(*_bound_args(c))
    print("noise_q100: bound", bound, "scan", len(c.ref.scan), "factor", bound / len(c.ref.scan))
    assert len(c.ref.scan) >= c.img.size and bound <= 7 * len(c.ref.scan)
    for args in ((0, 8, 3, 0, 1), (8, 8, 2, 0, 1), (8, 8, 4, 0, 1), (8, 8, 1, 1, 1), (8, 8, 3, 2, 1), (8, 8, 3, 0, 0), (8, 8, 3, 0, 65536), (65536, 8, 3, 0, 1)):
        assert L.rayn_jpeg_scan_bound(*args) == 0 and L.rayn_jpeg_scratch_bytes(*args) == 0, args


def test_categories_stay_inside_the_tables_on_the_extremal_blocks():
    """The block that maximises |F[v][u]| is the sign pattern of T[v][y] T[u][x]; both of its polarities, for each of the 64 basis functions,
    at quality 100: no AC size above 10, no DC difference category above 11 (encode_block asserts both) - and they are reached"""
    blocks = []
    for v in range(8):
        for u in range(8):
            pattern = np.outer(J.T[v], J.T[u]) > 0
            blocks += [np.where(pattern, 255, 0), np.where(pattern, 0, 255)]
    img = np.concatenate(blocks, axis=1).astype(np.uint8)[..., None]
    e = J.encode(img, 100, 0, 65535)
    assert max(s[0] for s in e.stats) == 11 and max(s[1] for s in e.stats) == 10
    assert np.abs(e.coef[:, 1:]).max() < 1024 and max(abs(int(a[0]) - int(b[0])) for a, b in zip(e.coef[1:], e.coef[:-1])) <= 2047


def test_jpeg_from_scan_frames_the_restatements_file_and_rejects_what_is_not_one(L):
    from rayn_amd import Jpeg, image
    for name in ("size_17x33_grey", "size_17x33_444", "size_17x33_420", "quality_1", "rst_wraps"):
        c = K.cases()[name]
        options = Jpeg(c.quality, "420" if c.subsampling else "444", c.ri)
        assert image.jpeg_from_scan(c.width, c.height, c.bpp, options, c.ref.encoded) == c.ref.file, name
        assert image.jpeg_from_scan(c.width, c.height, c.bpp, options, np.frombuffer(c.ref.encoded + b"\xa5" * 7, np.uint8)) == c.ref.file
    grey = K.cases()["size_17x33_grey"]
    assert image.jpeg_from_scan(17, 33, 1, Jpeg(75, "420", 2), grey.ref.encoded) == grey.ref.file  # a grey image has one form
    c = K.cases()["size_17x33_444"]
    good = Jpeg(75, "444", 2)
    for args, text in (((17, 33, 4, good, c.ref.encoded), "no alpha"), ((17, 33, 2, good, c.ref.encoded), "1 or 3"),
                       ((17, 33, 3, "90", c.ref.encoded), "must be a Jpeg"), ((0, 33, 3, good, c.ref.encoded), "1..65535"),
                       ((17, 33, 3, good, c.ref.encoded[:12]), "less than the header"), ((17, 33, 3, good, c.ref.encoded[:40]), "length word"),
                       ((17, 33, 3, Jpeg(75, "444", 3), c.ref.encoded), "not the scan of"), ((17, 33, 3, Jpeg(75, "420", 2), c.ref.encoded), "not the scan of"),
                       ((17, 41, 3, good, c.ref.encoded), "not the scan of")):
        with pytest.raises(ValueError, match=text):
            image.jpeg_from_scan(*args)
    for bad in (dict(quality=0), dict(quality=101), dict(quality=90.0), dict(subsampling="422"), dict(restart=0), dict(restart=65536)):
        with pytest.raises(ValueError):
            Jpeg(**bad)


def _three_frames():
    return [K.cases()[n].ref.file for n in ("size_17x33_444", "size_17x33_420", "size_17x33_grey")]


def test_avi_writer_against_a_reader_written_from_the_layout(tmp_path):
    from rayn_amd import image
    frames = _three_frames()
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames), "one odd and one even frame are the point"
    path = tmp_path / "a.avi"
    w = image.AviWriter(str(path), 17, 33, 24)
    for f in frames:
        w.add(f)
    w.close()
    w.close()  # twice is once
    a = avi_read.read(path.read_bytes())  # checks every chunk size, the even padding and the RIFF size on its way
    assert a["frames"] == frames
    assert a["avih"][4] == 3 and a["avih"][3] == 0x10 and a["avih"][6] == 1 and a["avih"][8:10] == (17, 33) and a["avih"][0] == round(1e6 / 24)
    assert a["strh"]["type"] == b"vids" and a["strh"]["handler"] == b"MJPG" and a["strh"]["length"] == 3
    assert (a["strh"]["rate"], a["strh"]["scale"]) == (24, 1) and a["strh"]["frame"] == (0, 0, 17, 33)
    assert a["strf"] == dict(size=40, width=17, height=33, planes=1, bits=24, compression=b"MJPG", image_bytes=17 * 33 * 3)
    assert a["avih"][7] == a["strh"]["buffer"] == max(len(f) for f in frames)
    assert len(a["index"]) == 3
    for (fourcc, flags, offset, size), at, f in zip(a["index"], a["frame_at"], frames):
        assert fourcc == b"00dc" and flags == 0x10 and a["movi_at"] + offset == at and size == len(f)
    for f in a["frames"]:
        Image.open(io.BytesIO(f)).load()
    rate = avi_read.read(_avi_bytes(tmp_path, image, frames[:1], 30000 / 1001))["strh"]
    assert (rate["rate"], rate["scale"]) == (30000, 1001)
    with pytest.raises(ValueError, match="closed"):
        w.add(frames[0])
    for bad in ((0, 33, 24), (17, 70000, 24), (17, 33, 0)):
        with pytest.raises(ValueError):
            image.AviWriter(str(tmp_path / "never.avi"), *bad)
    assert not (tmp_path / "never.avi").exists()


def _avi_bytes(tmp_path, image, frames, rate):
    p = tmp_path / "b.avi"
    with image.AviWriter(str(p), 17, 33, rate) as w:
        for f in frames:
            w.add(f)
    return p.read_bytes()


def test_avi_writer_closes_at_its_size_limit_and_after_an_exception(tmp_path, monkeypatch):
    from rayn_amd import image
    frames = _three_frames()
    # the limit: room for two frames, their chunk headers, the index of three and its header, but not for the third frame
    two = 224 + sum(8 + len(f) + (len(f) & 1) for f in frames[:2])
    monkeypatch.setattr(image.AviWriter, "LIMIT", two + 8 + 16 * 3 + 8 + len(frames[2]) - 1)
    path = tmp_path / "limit.avi"
    w = image.AviWriter(str(path), 17, 33, 24)
    w.add(frames[0])
    w.add(frames[1])
    with pytest.raises(ValueError, match="past"):
        w.add(frames[2])
    a = avi_read.read(path.read_bytes())  # finalised: two frames that play
    assert a["frames"] == frames[:2] and a["avih"][4] == a["strh"]["length"] == 2 and len(path.read_bytes()) <= image.AviWriter.LIMIT
    monkeypatch.undo()
    path = tmp_path / "raised.avi"
    with pytest.raises(RuntimeError, match="mid-sequence"):
        with image.AviWriter(str(path), 17, 33, 24) as w:
            w.add(frames[0])
            raise RuntimeError("mid-sequence")
    a = avi_read.read(path.read_bytes())
    assert a["frames"] == frames[:1] and a["avih"][4] == 1


def test_the_package_does_not_import_pil():
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = "import sys; import rayn_amd, rayn_amd.image, rayn_amd.film; assert not [m for m in sys.modules if m == 'PIL' or m.startswith('PIL.')]"
    subprocess.run([sys.executable, "-c", code], check=True, cwd=root, timeout=300)
