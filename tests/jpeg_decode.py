"""What the CPU tests of the JPEG cases (tests/test_jpeg.py, tests/test_jpeg_edge_cases.py) share: Pillow's decode of a file and the bounds
on libjpeg's reconstruction against the float64 reconstruction of the restatement's coefficients.  TEST INFRASTRUCTURE: nothing under
rayn_amd/ imports this."""
import io

import numpy as np
from PIL import Image  # the decoder the files are pinned against: its absence is a failure, not a skip

import jpeg_np as J


def decode(data, raw):
    """Pillow's decode of a file: raw = the planes libjpeg reconstructs (YCbCr without the colour conversion, or L)"""
    im = Image.open(io.BytesIO(data))
    if raw and im.mode != "L":
        im.draft("YCbCr", im.size)
    im.load()
    return im


# The largest difference between libjpeg's reconstruction (Pillow 12.2, libjpeg-turbo, its default integer inverse DCT) and the float64
# reconstruction of the restatement's own coefficients, measured here over every case of jpeg_cases on every full-resolution plane: 1.
PLANE_BOUND = 1
# The 4:2:0 chroma.  How a decoder upsamples is its own business: libjpeg's default ("fancy") h2v2 upsampling is the triangle filter - every
# output sample is (9 nearest + 3 + 3 + 1 next) / 16 of the chroma samples, edges replicated - so the decoded Cb / Cr, box-averaged back
# over the 2x2 samples of a chroma sample (float64, whole groups only), is the subsampled plane under the separable kernel (1 6 1) / 8,
# not the plane itself (against the plane itself the difference reaches 29 on the noise cases here, 1 on the smooth 8x8 ones).  Against
# that kernel applied to the float64 reconstruction of the restatement's subsampled planes the largest difference measured here over the
# 4:2:0 cases is 0.78.  Asserted: 1.5 - a decoded sample is within 1 of the exact one (PLANE_BOUND) and the upsampler rounds once more,
# 0.5, and the mean of four keeps at most that; a wrong plane (Cb for Cr, a block out of place, a shifted box) gives tens.
CHROMA_BOUND = 1.5


def _triangle_then_box(p):
    q = np.pad(p, 1, mode="edge")
    v = (q[:-2] + 6 * q[1:-1] + q[2:]) / 8
    return (v[:, :-2] + 6 * v[:, 1:-1] + v[:, 2:]) / 8


def reconstruction_differences(c):
    e, im = c.ref, decode(c.ref.file, True)
    got = np.asarray(im).astype(np.int64).reshape(c.height, c.width, -1)
    rec = J.reconstruct(e)
    full = [np.abs(got[..., 0] - rec[0][:c.height, :c.width]).max()]
    if c.bpp == 3 and not c.subsampling:
        full += [np.abs(got[..., k] - rec[k][:c.height, :c.width]).max() for k in (1, 2)]
    chroma = []
    if c.subsampling:
        ch, cw, hh, hw = -(-c.height // 2), -(-c.width // 2), c.height // 2, c.width // 2  # the chroma planes' size; whole 2x2 groups only
        for k in (1, 2):
            box = got[:2 * hh, :2 * hw, k].reshape(hh, 2, hw, 2).mean(axis=(1, 3))
            chroma.append(float(np.abs(box - _triangle_then_box(rec[k][:ch, :cw])[:hh, :hw]).max()) if hh and hw else 0.0)
    return full, chroma
