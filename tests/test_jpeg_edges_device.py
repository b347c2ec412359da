"""The device JPEG encoder at its decision edges: every case of tests/jpeg_edge_cases.py through every entry it applies to, byte for byte
against the restatement (tests/jpeg_np.py).  Image cases go through rayn_hip_jpeg_encode_device (output and scratch between guards) and
through rayn_hip_probe_jpeg_transform, whose coefficients are compared with the restatement's one by one, so that a transform difference
is reported as a coefficient and not as a scan offset.  Every case - an image case with the restatement's coefficients - goes through
rayn_hip_probe_jpeg_entropy with the scratch and the output pre-filled with 0x00, 0xFF and 0xA5: the encoder has no memset and must write
the same bytes whatever they held.  stale_buffers encodes two images one after the other into buffers that are not refilled."""
import ctypes as C
import struct

import numpy as np
import pytest

import device_io as IO
import jpeg_edge_cases as E

pytestmark = pytest.mark.gpu

GUARD = 0xA5


def _buffers(c):
    """(bound, scratch bytes, the guarded output pair, the guarded scratch pair) for a case's geometry"""
    import torch
    from rayn_amd import film as F
    args = (c.width, c.height, c.bpp, c.subsampling, c.ri)
    bound, need = F.jpeg_scan_bound(*args), F.jpeg_scratch_bytes(*args)
    assert bound and need and bound % 16 == 0 and need % 16 == 0
    return bound, need, IO.guarded(bound, torch.uint8, GUARD), IO.guarded(need, torch.uint8, GUARD)


def _encode_into(ctx, c, bound, need, out_pair, scr_pair):
    """The entry on case c into (possibly larger) buffers between guards: the whole output buffer as the device left it"""
    import torch
    d_img = IO.upload_bytes(c.img)
    ctx.jpeg_encode(c.width, c.height, c.bpp, d_img, out_pair[1], c.quality, c.subsampling, c.ri, scr_pair[1])
    torch.cuda.synchronize()
    IO.assert_guards(out_pair[0], bound, GUARD, "d_out")
    IO.assert_guards(scr_pair[0], need, GUARD, "d_scratch")
    IO.assert_is_host(d_img, c.img, "d_img", np.uint8)
    return out_pair[1].cpu().numpy()


def _written(got, bound):
    n = int(got[:4].view("<u4")[0])
    assert 1 <= n <= bound - 16, n
    return 16 + (n + 3) // 4 * 4


def _assert_encoded(name, got, want, header):
    if got != want:
        first = next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
        raise AssertionError((name, "header", struct.unpack("<4I", got[:16]), header, "first difference at byte", first, got[first:first + 8].hex(), want[first:first + 8].hex()))


@pytest.mark.parametrize("name", E.IMAGE_NAMES)
def test_an_image_case_through_the_entry(gpu_ctx, name):
    c = E.case(name)
    bound, need, out_pair, scr_pair = _buffers(c)
    got = _encode_into(gpu_ctx, c, bound, need, out_pair, scr_pair)
    written = _written(got, bound)
    assert np.all(got[written:] == GUARD), "bytes behind the scan's last word were written"
    _assert_encoded(name, got[:written].tobytes(), c.ref.encoded, c.ref.header)


@pytest.mark.parametrize("name", E.IMAGE_NAMES)
def test_an_image_case_through_the_transform_probe(gpu_ctx, name):
    from rayn_amd import _lib
    c = E.case(name)
    img = np.ascontiguousarray(c.img)
    got = np.full(c.ref.coef.shape, 0x7EEE, np.int16)
    rc = _lib.lib().rayn_hip_probe_jpeg_transform(gpu_ctx.h, c.width, c.height, c.bpp, c.quality, c.subsampling, img.ctypes.data_as(C.c_void_p), got.ctypes.data_as(C.c_void_p))
    assert rc == 0, gpu_ctx.last_error()
    bad = np.argwhere(got != c.ref.coef)
    assert not len(bad), (name, len(bad), "coefficients differ; the first: (block, zigzag position, device, restatement)",
                          [(int(b), int(k), int(got[b, k]), int(c.ref.coef[b, k])) for b, k in bad[:4]])


def _entropy_probe(ctx, c, coef, fill):
    from rayn_amd import _lib
    from rayn_amd import film as F
    bound = F.jpeg_scan_bound(c.width, c.height, c.bpp, c.subsampling, c.ri)
    coef = np.ascontiguousarray(coef, np.int16)
    out = np.full(bound + 16, 0x3C, np.uint8)   # 16 bytes of the host's own behind what the probe may write
    rc = _lib.lib().rayn_hip_probe_jpeg_entropy(ctx.h, c.width, c.height, c.bpp, c.subsampling, c.ri, coef.ctypes.data_as(C.c_void_p), fill,
                                                out.ctypes.data_as(C.c_void_p), bound)
    return rc, out, bound


@pytest.mark.parametrize("name", E.NAMES)
def test_every_case_through_the_entropy_probe_whatever_the_buffers_held(gpu_ctx, name):
    c = E.case(name)
    results = []
    for fill in E.FILL_BYTES:
        rc, out, bound = _entropy_probe(gpu_ctx, c, c.ref.coef, fill)
        assert rc == 0, (fill, gpu_ctx.last_error())
        assert np.all(out[bound:] == 0x3C)
        written = _written(out, bound)
        _assert_encoded((name, "fill", fill), out[:written].tobytes(), c.ref.encoded, c.ref.header)
        assert np.all(out[written:bound] == fill), (name, fill, "bytes behind the scan's last word were written")
        results.append(out[:written].tobytes())
    assert results[0] == results[1] == results[2]


def test_stale_buffers_a_second_encode_into_what_the_first_left(gpu_ctx):
    big, small = E.stale_pair()
    bound, need, out_pair, scr_pair = _buffers(big)
    small_bound = _buffers(small)[0]
    assert small_bound < bound
    for first, second in ((big, small), (small, big), (big, small)):   # the buffers are never refilled: the third encode sees both
        for c in (first, second):
            got = _encode_into(gpu_ctx, c, bound, need, out_pair, scr_pair)
            written = _written(got, bound)
            _assert_encoded((c.name, "behind", first.name), got[:written].tobytes(), c.ref.encoded, c.ref.header)
    # the last encode was the small image's: behind its prefix lies what the large one wrote, not the guard byte
    assert written < len(big.ref.encoded) and got[written:len(big.ref.encoded)].tobytes() == big.ref.encoded[written:]


def test_the_probes_reject_what_the_kernels_could_not_code(gpu_ctx):
    from rayn_amd import _lib
    L = _lib.lib()
    c = E.case("category_edges/grey")
    for at, value in (((0, 0), 1024), ((3, 0), -1025), ((0, 1), 1024), ((5, 63), -1024), ((len(c.coef) - 1, 63), 32767)):
        coef = np.array(c.coef)
        coef[at] = value
        rc, out, bound = _entropy_probe(gpu_ctx, c, coef, 0xA5)
        assert rc == -1 and "cannot produce" in gpu_ctx.last_error(), (at, value)
        assert np.all(out == 0x3C)
    coef = np.array(c.coef)
    coef[0, 0], coef[1, 0], coef[2, 5] = -1024, 1023, -1023   # the reach itself is accepted
    assert _entropy_probe(gpu_ctx, c, coef, 0xA5)[0] == 0, gpu_ctx.last_error()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    good = np.ascontiguousarray(c.coef)
    out = np.zeros(1 << 18, np.uint8)
    bound = _entropy_probe(gpu_ctx, c, good, 0)[2]
    assert bound <= len(out)
    for args, text in (((c.width, 8, 1, 0, 1, None, 0, vp(out), bound), "null buffer"), ((c.width, 8, 1, 0, 1, vp(good), 0, None, bound), "null buffer"),
                       ((c.width, 8, 1, 0, 1, vp(good), 256, vp(out), bound), "fill_byte"), ((c.width, 8, 1, 0, 1, vp(good), 0, vp(out), bound - 1), "rayn_jpeg_scan_bound"),
                       ((0, 8, 1, 0, 1, vp(good), 0, vp(out), bound), "zero-sized"), ((c.width, 8, 2, 0, 1, vp(good), 0, vp(out), bound), "bpp must be 1 or 3"),
                       ((c.width, 8, 1, 1, 1, vp(good), 0, vp(out), bound), "4:2:0 needs"), ((c.width, 8, 1, 0, 0, vp(good), 0, vp(out), bound), "restart_interval"),
                       ((8200, 8200, 1, 0, 65535, vp(good), 0, vp(out), bound), "out of range")):
        assert L.rayn_hip_probe_jpeg_entropy(gpu_ctx.h, *args) == -1, args
        assert text in gpu_ctx.last_error(), (args, gpu_ctx.last_error())
    assert L.rayn_hip_probe_jpeg_entropy(None, c.width, 8, 1, 0, 1, None, 0, None, 0) == -1
    img, coef = np.zeros((8, 8, 1), np.uint8), np.zeros(64, np.int16)
    for args, text in (((8, 8, 1, 0, 0, vp(img), vp(coef)), "quality"), ((8, 8, 1, 101, 0, vp(img), vp(coef)), "quality"), ((8, 8, 1, 50, 0, None, vp(coef)), "null buffer"),
                       ((8, 8, 1, 50, 0, vp(img), None), "null buffer"), ((8, 0, 1, 50, 0, vp(img), vp(coef)), "zero-sized"), ((8, 8, 4, 50, 0, vp(img), vp(coef)), "bpp must be 1 or 3"),
                       ((8, 8, 1, 50, 1, vp(img), vp(coef)), "4:2:0 needs"), ((8200, 8200, 1, 50, 0, vp(img), vp(coef)), "out of range")):
        assert L.rayn_hip_probe_jpeg_transform(gpu_ctx.h, *args) == -1, args
        assert text in gpu_ctx.last_error(), (args, gpu_ctx.last_error())
    assert L.rayn_hip_probe_jpeg_transform(None, 8, 8, 1, 50, 0, None, None) == -1
    assert L.rayn_hip_probe_jpeg_transform(gpu_ctx.h, 8, 8, 1, 100, 0, vp(img), vp(coef)) == 0 and int(coef[0]) == -1024 and not coef[1:].any()
