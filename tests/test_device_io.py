"""tests/device_io.py on CPU tensors: every assertion the device tests of the post-process entries lean on passes on clean data and raises
on the one word that is wrong - a guard element at either end or right behind the output, one flipped input bit, one mantissa bit, a
missing plane - and the two bit comparisons treat NaNs as they say.  No GPU."""
import numpy as np
import pytest
import torch

import device_io as IO
from common import bits_equal

f32 = np.float32
CPU = "cpu"


def _nan(bits):
    return np.array([bits], np.uint32).view(f32)


@pytest.mark.parametrize("dtype,fill", [(torch.float32, 7.0), (torch.uint8, 0xA5), (torch.int32, -3)])
@pytest.mark.parametrize("n", [0, 37])
@pytest.mark.parametrize("guard", [16, 64])
def test_guards(dtype, fill, n, guard):
    full, out = IO.guarded(n, dtype, fill, guard, device=CPU)
    assert full.numel() == n + guard and out.numel() == n and (n == 0 or out.data_ptr() == full.data_ptr()) and bool(torch.all(full == fill))
    out.fill_(1)  # what the kernel may write
    IO.assert_guards(full, n, fill, "clean")
    for at in (n, n + guard - 1, n + guard // 2):  # right behind the output, the last guard element, one in between
        hurt = full.clone()
        hurt[at] = 1
        with pytest.raises(AssertionError):
            IO.assert_guards(hurt, n, fill, at)
    # a bound that leaves nothing to look at is an error, not a pass
    with pytest.raises(AssertionError):
        IO.assert_guards(full, n + guard, fill, "vacuous")


def test_uploads_are_flat_copies():
    a = np.arange(24, dtype=np.float64).reshape(2, 3, 4)[:, ::-1]  # not contiguous, not float32
    t = IO.upload(a, device=CPU)
    assert t.dtype == torch.float32 and t.shape == (24,) and np.array_equal(t.numpy(), a.astype(f32).reshape(-1))
    b = np.ones(5, f32)
    t, tb = IO.upload(b, device=CPU), IO.upload_bytes(b, device=CPU)
    b[:] = 2.0  # the host array afterwards: the tensors do not follow
    assert bool(torch.all(t == 1.0)) and tb.dtype == torch.uint8 and np.array_equal(tb.numpy().view(f32), np.ones(5, f32))
    obj = np.array([0, 1, 0xFFFFFFFF], np.uint32)
    g = IO.upload_gbuffer(np.zeros((3, 4), f32), obj, device=CPU)
    assert sorted(g) == ["object", "records"] and g["object"].dtype == torch.int32 and g["object"].tolist() == [0, 1, -1] and g["records"].shape == (12,)
    film = {"color": np.zeros((3, 3), f32), "alpha": None, "normal": np.ones((3, 3), f32)}
    assert sorted(IO.upload_film(film, device=CPU)) == ["color", "normal"]
    assert sorted(IO.upload_film(film, ("color", "alpha", "background"), device=CPU)) == ["color"]


def test_unchanged_inputs():
    rng = np.random.default_rng(0)
    host = {"color": rng.normal(size=(11, 3)).astype(f32), "normal": rng.normal(size=(11, 3)).astype(f32)}
    host["color"][2, 1] = np.nan  # compared as bits: a NaN is equal to itself
    obj = rng.integers(0, 2 ** 32, 11, dtype=np.uint32)
    d, g = IO.upload_film(host, device=CPU), IO.upload_gbuffer(rng.normal(size=(11, 4)), obj, device=CPU)
    for tensors in (d, [d["color"], None, g["object"]]):
        snap = IO.snapshot(tensors)
        IO.assert_unchanged(tensors, snap, "clean")
    IO.assert_is_host(d["color"], host["color"], "clean")
    IO.assert_is_host(g["object"], obj, "clean", np.uint32)
    # one bit of one word, after the snapshot
    snap = IO.snapshot(d)
    d["normal"].view(torch.int32)[17] ^= 1
    with pytest.raises(AssertionError):
        IO.assert_unchanged(d, snap, "one bit")
    with pytest.raises(AssertionError):
        IO.assert_is_host(d["normal"], host["normal"], "one bit")
    IO.assert_is_host(d["color"], host["color"], "the other plane")
    g["object"][10] ^= 1 << 31
    with pytest.raises(AssertionError):
        IO.assert_gbuffer_is_host(g, np.zeros((11, 4), f32), obj, "sign bit of an object")


def test_the_two_comparators():
    rng = np.random.default_rng(1)
    a = rng.normal(size=(9, 3)).astype(f32)
    a[0, 0], a[1, 1], a[2, 2] = np.inf, -0.0, _nan(0x7FC00000)[0]
    for strict in (False, True):
        IO.assert_bits_equal(a, a.copy(), "clean", strict)
        IO.assert_planes_equal({"x": a, "y": a[:, 0]}, {"x": a.copy(), "y": a[:, 0].copy()}, "clean", strict)
        b = a.copy()
        b.view(np.uint32)[4, 1] ^= 1  # one mantissa bit
        with pytest.raises(AssertionError, match=r"'bit', 1,"):
            IO.assert_bits_equal(a, b, "bit", strict)
        with pytest.raises(AssertionError):
            IO.assert_planes_equal({"x": a, "y": a}, {"x": a, "y": b}, "bit", strict)
        with pytest.raises(AssertionError):
            IO.assert_planes_equal({"x": a}, {"x": a, "y": a}, "keys", strict)
        with pytest.raises(AssertionError):
            IO.assert_planes_equal({"x": a, "z": a}, {"x": a, "y": a}, "keys", strict)
        z = a.copy()
        z[1, 1] = 0.0  # +0 against -0
        with pytest.raises(AssertionError):
            IO.assert_bits_equal(a, z, "zero", strict)
        with pytest.raises(AssertionError):
            IO.assert_bits_equal(a, a[:8], "shape", strict)
    # NaNs: the sign and the payload count under the strict comparator only; a NaN against a number fails under both
    for other in (0xFFC00000, 0x7FC00001, 0x7F800001):
        x, y = _nan(0x7FC00000), _nan(other)
        assert bits_equal(x, y) and not IO.same_bits(x, y)
        IO.assert_bits_equal(x, y, "payload")
        with pytest.raises(AssertionError):
            IO.assert_bits_equal(x, y, "payload", strict=True)
    for strict in (False, True):
        for number in (0.0, 1.0, np.inf):
            with pytest.raises(AssertionError):
                IO.assert_bits_equal(_nan(0x7FC00000), np.array([number], f32), "NaN against a number", strict)
            with pytest.raises(AssertionError):
                IO.assert_bits_equal(np.array([number], f32), _nan(0xFFC00000), "a number against NaN", strict)
    assert IO.same_bits(a, a.copy()) and not IO.same_bits(a, a[:8]) and not bits_equal(_nan(0x7FC00000), np.zeros(1, f32))


def test_read_folder(tmp_path):
    (tmp_path / "b.bin").write_bytes(b"\x00\x01")
    (tmp_path / "a.bin").write_bytes(b"xyz")
    assert IO.read_folder(tmp_path) == {"a.bin": b"xyz", "b.bin": b"\x00\x01"} and list(IO.read_folder(str(tmp_path))) == ["a.bin", "b.bin"]
