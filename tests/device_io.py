"""What the device tests of the post-process entries share: host arrays to the device and back, outputs between guard words, inputs left
alone, the two bit comparisons, and the module-scoped context.  Every function takes `device`, so that tests/test_device_io.py can hold
the assertions themselves to account on CPU tensors.  TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import os

import numpy as np
import pytest

from common import bits_equal

f32 = np.float32


@pytest.fixture(scope="module")
def module_context():
    """A context of the importing module's own (`from device_io import module_context as ctx`): its tests switch the mul_add policy and
    upload their worlds."""
    import rayn_amd
    c = rayn_amd.Context(0)
    yield c
    c.close()


# ---- uploads: always a contiguous, flattened copy ------------------------------------------------------------------------------------------

def upload(a, dtype=f32, device="cuda"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype).reshape(-1).copy()).to(device)


def upload_bytes(a, device="cuda"):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).to(device)


def upload_gbuffer(rec, obj, device="cuda"):
    """{"records", "object"} as rayn_amd.film.alloc_gbuffer lays them out: the objects are the int32 view of the uint32 ids"""
    return {"records": upload(rec, device=device), "object": upload(np.ascontiguousarray(obj, np.uint32).view(np.int32), np.int32, device)}


def upload_film(film, keys=None, device="cuda"):
    """The planes of `film` (all of them, or those of `keys`) that are present and not None"""
    return {k: upload(film[k], device=device) for k in (film if keys is None else keys) if film.get(k) is not None}


# ---- outputs between guard words -----------------------------------------------------------------------------------------------------------

def guarded(n, dtype, fill, guard=64, device="cuda"):
    """(the whole buffer of n + guard elements, all `fill`; its first n elements, the view a kernel is handed)"""
    import torch
    full = torch.full((n + guard,), fill, dtype=dtype, device=device)
    return full, full[:n]


def assert_guards(full, n, fill, what):
    """Everything of `full` behind its first n elements still holds `fill`; n = 0 is the output that was not handed over at all."""
    import torch
    assert 0 <= n < full.numel(), (what, "no guard element to look at")
    assert bool(torch.all(full[n:] == fill)), (what, "a kernel wrote past the output or into an absent one")


# ---- inputs left alone ---------------------------------------------------------------------------------------------------------------------

def _present(tensors):
    items = tensors.items() if isinstance(tensors, dict) else enumerate(tensors)
    return [(k, t) for k, t in items if t is not None]


def snapshot(tensors):
    """Clones of a dict's or a sequence's tensors (None entries are skipped), for assert_unchanged after the call"""
    return [t.clone() for _, t in _present(tensors)]


def assert_unchanged(tensors, snap, what):
    """Bit for bit, on integer views: the buffers hold NaNs"""
    import torch
    now = _present(tensors)
    assert len(now) == len(snap), what
    for (k, t), keep in zip(now, snap):
        assert torch.equal(t.reshape(-1).view(torch.uint8), keep.reshape(-1).view(torch.uint8)), (what, k, "was modified")


def assert_is_host(tensor, host_array, what, dtype=f32):
    """The device buffer still holds the bytes of the host array it was uploaded from (read as `dtype`)"""
    got = tensor.cpu().numpy().reshape(-1).view(np.uint8)
    assert np.array_equal(got, np.ascontiguousarray(host_array, dtype).reshape(-1).view(np.uint8)), (what, "was modified")


def assert_gbuffer_is_host(g, rec, obj, what):
    assert_is_host(g["records"], rec, (what, "records"))
    assert_is_host(g["object"], obj, (what, "object"), np.uint32)


# ---- bit comparison: common.bits_equal (two NaNs are equal whatever their payload) and the strict same_bits --------------------------------

def same_bits(a, b):
    """Every 32-bit word equal, NaN payloads and the sign of zero included"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def assert_bits_equal(got, want, what, strict=False):
    """float32 arrays under one of the two comparators; a failure names how many words differ"""
    got, want = np.ascontiguousarray(got, f32), np.ascontiguousarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if not (same_bits(got, want) if strict else bits_equal(got, want)):
        bad = got.view(np.uint32) != want.view(np.uint32)
        if not strict:
            bad &= ~(np.isnan(got) & np.isnan(want))
        raise AssertionError((what, int(bad.sum()), got[bad][:4], want[bad][:4]))


def assert_planes_equal(got, want, what, strict=False):
    """Two dicts of planes: the same keys, every plane bit-equal"""
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        assert_bits_equal(got[k], want[k], (what, k), strict)


# ---- what several modules do with a context ------------------------------------------------------------------------------------------------

def read_folder(folder):
    return {f: open(os.path.join(folder, f), "rb").read() for f in sorted(os.listdir(folder))}


def gpu_gbuffer(ctx, p):
    """Context.gbuffer of the uploaded world -> (device G-buffer, records (n, 4), objects (n,) uint32)"""
    import torch
    from rayn_amd import film as F
    g = F.alloc_gbuffer(p.width, p.height, "cuda")
    ctx.gbuffer(p, g)
    torch.cuda.synchronize()
    return g, g["records"].cpu().numpy().reshape(-1, 4), g["object"].cpu().numpy().view(np.uint32)


def render_frames(ctx, wd, ps, bounces):
    """Uploads the world and renders one device film per frame-parameter set, with the frame's default tables"""
    import torch
    import rayn_amd as R
    ctx.upload_world(wd)
    frames = []
    for p in ps:
        tabs = R.build_tables(4 * p.samples, bounces, p.volume_marches, p.frame, p.width, p.height)
        out = R.film.alloc_device_film(p.width, p.height, "cuda")
        ctx.render_device(p, [torch.from_numpy(t).cuda() for t in tabs], out)
        torch.cuda.synchronize()
        frames.append(out)
    return frames


def png_bytes(tmp_path, img):
    """The bytes rayn_amd.image.save writes for an image"""
    from rayn_amd import image
    p = tmp_path / "ref.png"
    image.save(str(p), img)
    return p.read_bytes()


def host_film(film):
    """The four planes of a rayn_amd.Film on the host, under the device films' keys"""
    K = type(film.channel_kinds[0])
    return {"color": film.channel(K.Color), "alpha": film.channel(K.Alpha), "background": film.channel(K.Background), "normal": film.channel(K.WorldNormal)}


def shutter_range(frame, rate=24, shutter=1.0 / 24.0):
    """The time range Film.render_sequence gives a frame, in its float32 arithmetic"""
    start = f32(frame) * (f32(1.0) / f32(rate))
    return float(start), float(f32(start + f32(shutter)))


def render_sequence_frame(ctx, w, h, frame, samples, bounces, filt):
    """A frame as Film.render_sequence renders it at 24 frames a second under the uploaded world: (frame parameters, device film)"""
    import torch
    import rayn_amd as R
    p = R.frame_params(w, h, samples, bounces, frame=frame, time_range=shutter_range(frame))
    out = R.film.alloc_device_film(w, h, "cuda")
    tabs = R.build_tables(4 * samples, bounces, p.volume_marches, frame, w, h, filt)
    ctx.render_device(p, [torch.from_numpy(t).cuda() for t in tabs], out)
    return p, out
