"""One rayn_ctx behind ctypes: Context, the byte-count and allocation helpers, the host table builders and the checks every device
entry's tensor arguments go through.  rayn_amd.film re-exports every name."""
import ctypes as C

import numpy as np

from . import _abi
from . import progressive as _prog
from ._lib import RaynHipError, lib
from .options import JPEG_DEFAULT_RESTART


def display_scratch_bytes(width, height, levels):
    """rayn_display_scratch_bytes: bytes of device scratch the display transform needs for a width x height film with `levels` bloom
    levels (0 for a size it rejects or levels > 8).  A manual exposure without bloom needs none."""
    return int(lib().rayn_display_scratch_bytes(int(width), int(height), int(levels)))


def gbuffer_scratch_bytes(width, height):
    """rayn_gbuffer_scratch_bytes: bytes of device scratch the G-buffer pass needs for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_gbuffer_scratch_bytes(int(width), int(height)))


def temporal_history_bytes(width, height):
    """rayn_temporal_history_bytes: bytes of one history of the temporal accumulation for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_temporal_history_bytes(int(width), int(height)))


def temporal_moments_bytes(width, height):
    """rayn_temporal_moments_bytes: bytes of the luminance moments beside one history (a float2 per pixel; 0 for a size the entries reject)."""
    return int(lib().rayn_temporal_moments_bytes(int(width), int(height)))


def preview_scratch_bytes(width, height, samples):
    """rayn_preview_scratch_bytes: bytes of device scratch the preview integrator needs for a width x height image with `samples` AO rays
    per pixel (0 for a size it rejects and for samples outside 1..64)."""
    return int(lib().rayn_preview_scratch_bytes(int(width), int(height), int(samples)))


def png_stream_bound(width, height, bpp):
    """rayn_png_stream_bound: the bytes Context.png_encode's output needs for a width x height image of `bpp` (1, 3 or 4) bytes per pixel:
    the 16-byte header and the longest zlib stream the encoder can write (0 for a geometry it rejects).  Host only."""
    return int(lib().rayn_png_stream_bound(int(width), int(height), int(bpp)))


def png_scratch_bytes(width, height, bpp):
    """rayn_png_scratch_bytes: bytes of device scratch the PNG encoder needs (0 for a geometry it rejects).  Host only."""
    return int(lib().rayn_png_scratch_bytes(int(width), int(height), int(bpp)))


def png_scratch_bytes_lz77(width, height, bpp):
    """rayn_png_scratch_bytes_lz77: bytes of device scratch Context.png_encode_lz77 needs (0 for a geometry it rejects).  Host only."""
    return int(lib().rayn_png_scratch_bytes_lz77(int(width), int(height), int(bpp)))


def _jpeg_args(width, height, bpp, subsampling, restart_interval):
    a = [int(width), int(height), int(bpp), int(subsampling), int(restart_interval)]
    return a if all(0 <= v < 1 << 32 for v in a) else None


def jpeg_scan_bound(width, height, bpp, subsampling, restart_interval):
    """rayn_jpeg_scan_bound: the bytes Context.jpeg_encode's output needs: the 16-byte header and the longest scan the tables allow, byte
    stuffing and restart markers included (0 for a geometry the encoder rejects).  Host only."""
    a = _jpeg_args(width, height, bpp, subsampling, restart_interval)
    return int(lib().rayn_jpeg_scan_bound(*a)) if a else 0


def jpeg_scratch_bytes(width, height, bpp, subsampling, restart_interval):
    """rayn_jpeg_scratch_bytes: bytes of device scratch the JPEG encoder needs (0 for a geometry it rejects).  Host only."""
    a = _jpeg_args(width, height, bpp, subsampling, restart_interval)
    return int(lib().rayn_jpeg_scratch_bytes(*a)) if a else 0


def jpeg_quant_table(quality, which):
    """rayn_jpeg_quant_table: the 64 entries of quantisation table `which` (0 luminance, 1 chrominance) at `quality`, in the zigzag order
    of a DQT segment, as bytes.  Host only."""
    out = (C.c_uint8 * 64)()
    if not (0 <= int(quality) < 1 << 32 and 0 <= int(which) < 1 << 32) or lib().rayn_jpeg_quant_table(int(quality), int(which), out) != 0:
        raise ValueError(f"no quantisation table {which!r} at quality {quality!r}: quality is 1..100, the table 0 or 1")
    return bytes(out)


def jpeg_huffman_table(which):
    """rayn_jpeg_huffman_table: (BITS, HUFFVAL) of Huffman table `which` (0 DC luminance, 1 AC luminance, 2 DC chrominance, 3 AC
    chrominance), as bytes, as a DHT segment holds them.  Host only."""
    bits, vals = (C.c_uint8 * 16)(), (C.c_uint8 * 256)()
    n = lib().rayn_jpeg_huffman_table(int(which), bits, vals, 256) if 0 <= int(which) < 1 << 32 else -1
    if n < 0:
        raise ValueError(f"no Huffman table {which!r}: 0..3")
    return bytes(bits), bytes(vals[:n])


def deflate_stream_bound(n):
    """rayn_deflate_stream_bound: the bytes Context.deflate's output needs for n input bytes: the 16-byte header and the longest zlib
    stream it can write (0 for n == 0 and n >= 2^31).  Host only."""
    return int(lib().rayn_deflate_stream_bound(int(n))) if 0 <= int(n) < 1 << 63 else 0


def deflate_scratch_bytes(n):
    """rayn_deflate_scratch_bytes: bytes of device scratch Context.deflate needs for n input bytes (0 for a size it rejects).  Host only."""
    return int(lib().rayn_deflate_scratch_bytes(int(n))) if 0 <= int(n) < 1 << 63 else 0


def _exr_layout(layout):
    """(n_channels, the 3 * n_channels words of rayn_hip_exr_encode_device's layout, or None) of (stride, offset, type) triples: sizes no
    32-bit word holds have no layout the entry accepts"""
    flat = [int(v) for triple in layout for v in triple]
    n = len(flat) // 3
    if len(flat) != 3 * n or any(not 0 <= v < 1 << 32 for v in flat):
        return n, None
    return n, (C.c_uint32 * max(len(flat), 1))(*flat)


def exr_stream_bound(width, height, layout):
    """rayn_exr_stream_bound: the bytes Context.exr_encode's output needs for a width x height image of the channels `layout` ((stride,
    offset, type) per channel): the four words, the chunk table and every chunk as raw bytes - exact, no payload is longer (0 for what
    the entry rejects).  Host only."""
    n, words = _exr_layout(layout)
    if words is None or not (0 <= int(width) < 1 << 32 and 0 <= int(height) < 1 << 32):
        return 0
    return int(lib().rayn_exr_stream_bound(int(width), int(height), n, words))


def exr_scratch_bytes(width, height, layout, lz77=False):
    """rayn_exr_scratch_bytes: bytes of device scratch Context.exr_encode needs (0 for what the entry rejects).  Host only."""
    n, words = _exr_layout(layout)
    if words is None or not (0 <= int(width) < 1 << 32 and 0 <= int(height) < 1 << 32):
        return 0
    return int(lib().rayn_exr_scratch_bytes(int(width), int(height), n, words, int(bool(lz77))))


def preview_tables(samples, frame, width, height):
    """The default tables of a preview of `samples` AO rays for frame `frame`: (the sample table (samples, 2) float32 - 2-D set 0 of
    build_rd_tables(samples, 0, 2, frame), so successive frames get different directions - and the per-pixel scramble of
    build_film_tables)."""
    s2 = build_rd_tables(int(samples), 0, 2, int(frame))[1]
    return np.ascontiguousarray(s2[: 2 * int(samples)].reshape(int(samples), 2)), build_film_tables(int(width), int(height))[0]


def alloc_gbuffer(width, height, device="cuda"):
    """The two planes of a G-buffer as Context.gbuffer fills them: records (n, 4) float32 (Px, Py, Pz, t) and object (n,) int32 (the u32
    object index; a miss is -1 = 0xFFFFFFFF)."""
    import torch
    n = width * height
    return {"records": torch.zeros(n, 4, dtype=torch.float32, device=device), "object": torch.zeros(n, dtype=torch.int32, device=device)}


def denoise_scratch_bytes(width, height):
    """rayn_denoise_scratch_bytes: bytes of device scratch the denoiser needs for a width x height film (0 for a size it rejects)."""
    return int(lib().rayn_denoise_scratch_bytes(int(width), int(height)))


def denoise_variance_scratch_bytes(width, height):
    """rayn_denoise_variance_scratch_bytes: bytes of device scratch the variance-guided denoiser needs for a width x height film (0 for a
    size it rejects)."""
    return int(lib().rayn_denoise_variance_scratch_bytes(int(width), int(height)))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def build_tables(spp, max_bounces, volume_marches, frame, width, height, filter=None):
    """Samples::new_rd (src/sampler.rs:18-37), per-pixel scramble (src/film.rs:460-461) and
    FilterImportanceSampler::new (src/filter.rs:196-220) through the product's host builders."""
    s1, s2 = build_rd_tables(spp, max_bounces, volume_marches, frame)
    scr, fis = build_film_tables(width, height, filter)
    return s1, s2, scr, fis


def build_rd_tables(spp, max_bounces, volume_marches, frame):
    """Samples::new_rd (src/sampler.rs:18-37): the only tables that depend on the frame."""
    L = lib()
    n1, n2 = L.rayn_sets_1d(max_bounces, volume_marches), L.rayn_sets_2d(max_bounces, volume_marches)
    s1, s2 = np.zeros(spp * n1, np.float32), np.zeros(spp * 2 * n2, np.float32)
    rc = L.rayn_build_rd_tables(spp, n1, n2, frame, _fp(s1), _fp(s2))
    if rc != 0:
        raise RaynHipError(f"table builder failed: {rc}")
    return s1, s2


def build_film_tables(width, height, filter=None):
    """The per-pixel scramble (src/film.rs:460-461) and FilterImportanceSampler::new (src/filter.rs:196-220)."""
    L = lib()
    kind, radius = (0, 1.5) if filter is None else (filter.kind, filter.radius)
    p0, p1 = getattr(filter, "params", (0.0, 0.0))
    scr, fis = np.zeros(width * height, np.float32), np.zeros(_abi.FIS_TABLE_SIZE, np.float32)
    for rc in (L.rayn_build_scramble(width, height, _fp(scr)), L.rayn_build_fis_table_ex(kind, radius, p0, p1, _fp(fis))):
        if rc != 0:
            raise RaynHipError(f"table builder failed: {rc}")
    return scr, fis


class RdTablePrefetch:
    """The device sample tables of a run of renders (the frames of a sequence, the epochs of a progressive render).  Only the R_d
    tables (Samples::new_rd) depend on the render: they are built on a host thread, one render ahead; scramble and filter tables are
    built once, while the first build runs.  `seeds`: the frame numbers or seeds of the renders, in order (any iterable; taken one
    at a time).  `pool`: a one-thread executor, which the caller shuts down in its `finally`."""

    def __init__(self, pool, seeds, spp, max_bounces, volume_marches, width, height, filter, device):
        self._pool, self._seeds, self._args, self._device = pool, iter(seeds), (spp, max_bounces, volume_marches), device
        self._submit()
        self._film_tables = build_film_tables(width, height, filter)
        self.d_tables = None

    def _submit(self):
        seed = next(self._seeds, None)
        self._next = None if seed is None else self._pool.submit(build_rd_tables, *self._args, seed)

    def next(self):
        """The device tables of the next render; the build for the one after it is started.  The first call uploads all four, later
        ones copy into the first two - synchronous copies from pageable memory, so the previous render must have returned."""
        import torch
        s1, s2 = self._next.result()
        self._submit()
        if self.d_tables is None:
            self.d_tables = [torch.from_numpy(t).to(self._device) for t in (s1, s2, *self._film_tables)]
        else:
            self.d_tables[0].copy_(torch.from_numpy(s1))
            self.d_tables[1].copy_(torch.from_numpy(s2))
        return self.d_tables


def share_pixels(params):
    """rayn_share_pixels: pixels of the tiles the share (params.tile_first, params.tile_step) owns; its packed film is 10 floats each."""
    return int(lib().rayn_share_pixels(C.byref(params)))


# The checks of the tensors a device entry takes.  Plain functions of torch tensors: none touches a Context or the GPU.

FILM_KEYS = ("color", "alpha", "background", "normal")
GUIDE_KEYS = ("color", "alpha", "normal")
_PLANE_FLOATS = {"color": 3, "alpha": 1, "background": 3, "normal": 3}


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _opt_ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def f32_ptr(t, label, floats):
    """The pointer of the float32 tensor `t`, which must be contiguous and hold at least `floats` elements; `label` names it in the
    ValueError."""
    import torch
    if t is None or not (t.dtype == torch.float32 and t.is_contiguous() and t.numel() >= floats):
        raise ValueError(f"{label} must be a contiguous float32 tensor of at least {floats} floats")
    return _ptr(t)


def opt_f32_ptr(t, label, floats):
    """f32_ptr, and None for None."""
    return None if t is None else f32_ptr(t, label, floats)


def i32_ptr(t, label, count):
    """As f32_ptr for an int32 tensor of at least `count` elements."""
    import torch
    if t is None or not (t.dtype == torch.int32 and t.is_contiguous() and t.numel() >= count):
        raise ValueError(f"{label} must be a contiguous int32 tensor of at least {count} elements")
    return _ptr(t)


def film_ptrs(d_film, keys, n, label):
    """The pointers of the planes `keys` of the film dict `d_film` of n pixels (3 / 1 / 3 / 3 floats a pixel), None for an absent one."""
    return [opt_f32_ptr(d_film.get(k), f"{label}[{k!r}]", _PLANE_FLOATS[k] * n) for k in keys]


def gbuffer_ptrs(d_gbuffer, n, label):
    """[records pointer, object pointer] of the G-buffer dict `d_gbuffer` of n pixels (alloc_gbuffer's); both planes are required."""
    return [f32_ptr(d_gbuffer.get("records"), f"{label}['records']", 4 * n), i32_ptr(d_gbuffer.get("object"), f"{label}['object']", n)]


def byte_ptrs(d_new, new_label, d_prev=None, prev_label=None):
    """(pointer of d_prev or None, pointer of d_new, bytes) of a pair of uint8 buffers one entry reads and writes (the histories, the
    moments) or of a single one (a progressive state): d_new is required, d_prev optional, and the byte count is the smaller of the two."""
    import torch
    for name, t in ((prev_label, d_prev), (new_label, d_new)):
        if t is not None and not (t.dtype == torch.uint8 and t.is_contiguous()):
            raise ValueError(f"{name} must be a contiguous uint8 tensor")
    if d_new is None:
        raise ValueError(f"{new_label} must be a contiguous uint8 tensor")
    return _opt_ptr(d_prev), _ptr(d_new), d_new.numel() if d_prev is None else min(d_new.numel(), d_prev.numel())


def scratch(d_scratch, nbytes, device):
    """(tensor, pointer, bytes) of an entry's scratch: `d_scratch`, which must be contiguous, or max(nbytes, 1) fresh bytes on
    `device` for None.  The caller holds the tensor until its entry has been enqueued."""
    import torch
    if d_scratch is None:
        d_scratch = torch.empty(max(int(nbytes), 1), dtype=torch.uint8, device=device)
    if not d_scratch.is_contiguous():
        raise ValueError("d_scratch must be contiguous")
    return d_scratch, _ptr(d_scratch), d_scratch.numel() * d_scratch.element_size()


def stream_ptr(stream):
    """The raw stream an entry enqueues on: `stream`, or torch's current one for None."""
    if stream is None:
        import torch
        stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(stream)


def _upscale_args(params, upscale, d_film, d_low_gbuffer, d_high_gbuffer, d_out_film, d_out_weight):
    """What upscale and temporal_upscale share: (the low film's planes, the low and the high G-buffer's planes, the high film's planes,
    the weight plane or None) as pointers, checked against the low size of `params` and upscale.factor times it."""
    n = int(params.width) * int(params.height)
    N = n * int(upscale.factor) ** 2
    low, high = film_ptrs(d_film, FILM_KEYS, n, "d_film"), film_ptrs(d_out_film, FILM_KEYS, N, "d_out_film")
    gp = gbuffer_ptrs(d_low_gbuffer, n, "d_low_gbuffer") + gbuffer_ptrs(d_high_gbuffer, N, "d_high_gbuffer")
    return low, gp, high, opt_f32_ptr(d_out_weight, "d_out_weight", N)


class Context:
    """One rayn_ctx (one GPU).  Fails loudly when the HIP library or a GPU is missing."""

    def __init__(self, device=0):
        """device: one GPU index, or a list of indices for a multi-device context (rayn_hip_create_multi; buffers passed
        to render_device then live on the first one)."""
        self._L = lib()
        h = C.c_void_p()
        if isinstance(device, (list, tuple)):
            ids = (C.c_int * len(device))(*device)
            rc = self._L.rayn_hip_create_multi(ids, len(device), C.byref(h))
            first = device[0] if len(device) else 0
        else:
            rc = self._L.rayn_hip_create(device, C.byref(h))
            first = device
        if rc != 0:
            raise RaynHipError(f"rayn_hip_create(device={device}) failed with {rc} (no usable GPU?)")
        self.h = h
        self.device = first
        self.fma_policy = int(self._L.rayn_hip_fma_policy())  # of this ctx: the library's default until set_fma_policy

    def device_count(self):
        return self._L.rayn_hip_device_count(self.h)

    def _chk(self, rc):
        if rc != 0:
            raise RaynHipError(f"rayn_hip error {rc}: {self._L.rayn_hip_last_error(self.h).decode()}")

    def table_broadcasts(self):
        """multi-device context: peer copies of the sample tables made so far (rayn_hip_table_broadcasts)"""
        return int(self._L.rayn_hip_table_broadcasts(self.h))

    def last_error(self):
        return self._L.rayn_hip_last_error(self.h).decode()

    def upload_world(self, desc):
        self._chk(self._L.rayn_hip_upload_world(self.h, C.byref(desc)))

    def set_profiling(self, timing=True, count_evals=False):
        self._chk(self._L.rayn_hip_set_profiling(self.h, int(timing), int(count_evals)))

    def set_fma_policy(self, policy):
        """0 = unfused mul_add (reference default build, the default), 1 = fused (rayn built with +fma)."""
        self._chk(self._L.rayn_hip_set_fma_policy(self.h, int(policy)))
        self.fma_policy = int(policy)

    def set_workers(self, n_workers, min_paths=1 << 22):
        self._chk(self._L.rayn_hip_set_workers(self.h, int(n_workers), int(min_paths)))

    def set_tile_subset(self, tiles=None):
        """Render only these tiles (reference tile order) until cleared with None / []."""
        arr = np.ascontiguousarray([] if tiles is None else tiles, dtype=np.uint32)
        self._chk(self._L.rayn_hip_set_tile_subset(self.h, arr.ctypes.data_as(C.POINTER(C.c_uint32)), len(arr)))

    def set_trace_tile(self, tile_index):
        self._chk(self._L.rayn_hip_set_trace_tile(self.h, int(tile_index)))

    def trace(self):
        """Packet-order dump of the traced tile: dict of uint32 arrays (depth, obj, px, py, sample, valid)."""
        n = self._L.rayn_hip_get_trace(self.h, None, 0)
        buf = np.zeros((max(n, 0), 6), np.uint32)
        if n > 0:
            self._L.rayn_hip_get_trace(self.h, buf.ctypes.data_as(C.POINTER(C.c_uint32)), n)
        return {k: buf[:, i].copy() for i, k in enumerate(("depth", "obj", "px", "py", "sample", "valid"))}

    def set_batch_paths(self, n):
        self._chk(self._L.rayn_hip_set_batch_paths(self.h, int(n)))

    def set_cold_bytes(self, n):
        """arena bytes of ALL workers together for the context's first frame (rayn_hip_set_cold_bytes, rayn_hip.h); 0 = full-size batches from the first frame"""
        self._chk(self._L.rayn_hip_set_cold_bytes(self.h, int(n)))

    def stats(self):
        s = _abi.Stats()
        self._chk(self._L.rayn_hip_get_stats(self.h, C.byref(s)))
        return s.as_dict()

    def entry_stats(self, entry):
        """What device `entry` of a multi-device context did in the last frame (rayn_hip_get_entry_stats)."""
        s = _abi.Stats()
        self._chk(self._L.rayn_hip_get_entry_stats(self.h, int(entry), C.byref(s)))
        return s.as_dict()

    def _counters(self, entry, names):
        out = (C.c_uint64 * len(names))()
        self._chk(entry(self.h, out))
        return dict(zip(names, out))

    def eval_counts(self):
        return self._counters(self._L.rayn_hip_get_eval_counts, ("extend", "shade_setup", "shadow"))

    def sdf_iterations(self):
        """Fold / orbit iterations run by the evaluations of eval_counts() (instrumented kernels, rayn_hip_get_sdf_iterations)."""
        return self._counters(self._L.rayn_hip_get_sdf_iterations, ("extend", "shade_setup", "shadow"))

    def elision_counts(self):
        """Instrumented kernels (rayn_hip_get_elision_counts): shaded slots with throughput exactly (0, 0, 0) whose NEE was elided, and the
        shadow segments they would have parked."""
        return self._counters(self._L.rayn_hip_get_elision_counts, ("zero_throughput_slots", "elided_shadow_jobs", "samples_out_of_bounds"))

    def stage_slots(self):
        """Instrumented Mandelbulb shadow-march kernel (rayn_hip_get_stage_slots): lane slots offered by the orbit / epilogue stage of k_shadow_bulb."""
        return self._counters(self._L.rayn_hip_get_stage_slots, ("shadow_orbit", "shadow_epilogue"))

    def render_host(self, params, tables, out=None):
        """rayn_hip_render_frame with host (numpy) buffers.  Returns the film dict."""
        s1, s2, scr, fis = tables
        n = params.width * params.height
        if out is None:
            out = {"color": np.zeros((n, 3), np.float32), "alpha": np.zeros(n, np.float32),
                   "background": np.zeros((n, 3), np.float32), "normal": np.zeros((n, 3), np.float32)}
        self._chk(self._L.rayn_hip_render_frame(self.h, C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), _fp(out["color"]),
                                                _fp(out["alpha"]), _fp(out["background"]), _fp(out["normal"])))
        h, w = params.height, params.width
        return {"color": out["color"].reshape(h, w, 3), "alpha": out["alpha"].reshape(h, w),
                "background": out["background"].reshape(h, w, 3), "normal": out["normal"].reshape(h, w, 3)}

    def probe_shade_limits(self):
        """(stream_blocks, list_ids_per_block, setup_threads): rayn_hip_probe_shade_limits."""
        v = [C.c_uint32() for _ in range(3)]
        self._chk(self._L.rayn_hip_probe_shade_limits(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def probe_scene_dispatch(self, params):
        """rayn_hip_probe_scene_dispatch (rayn_hip.h): what the values of the uploaded world and `params` decide, from the build_scene and scene_march_kernels
        a render calls.  -> dict: single_sdf (index or -1), sdf_kind (-1, 0, 1, 2, 100), bulb, anim_spheres, fast_div (list, one entry per hitable)."""
        out = (C.c_int32 * (4 + _abi.MAX_HITABLES))()
        self._chk(self._L.rayn_hip_probe_scene_dispatch(self.h, C.byref(params), out))
        v = list(out)
        return {"single_sdf": v[0], "sdf_kind": v[1], "bulb": v[2], "anim_spheres": v[3], "fast_div": [x for x in v[4:] if x >= 0]}

    def probe_sdf_dist_as(self, params, hitable_index, sdfk, fast_div, pts, t0=0.0, out=None, check=True):
        """rayn_hip_probe_sdf_dist_as (rayn_hip.h): sdf_dist<false, sdfk> of one TracedSDF in the division arm `fast_div` at the packet time t0, per point of
        pts [n, 3].  -> (rc, out [n] float32); `out` may be handed in to see that a refused call leaves it alone.  check=False returns a non-zero rc instead of raising."""
        pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
        if out is None:
            out = np.zeros(len(pts), np.float32)
        assert out.dtype == np.float32 and out.size == len(pts) and out.flags.c_contiguous
        rc = self._L.rayn_hip_probe_sdf_dist_as(self.h, C.byref(params), int(hitable_index), int(sdfk), int(fast_div), float(t0), _fp(pts), _fp(out), len(pts))
        if check:
            self._chk(rc)
        return rc, out

    RAYGEN_CTL = ("q_groups", "q_valid", "b_groups", "b_valid", "head_extend", "job_count", "head_shadow", "overflow")

    def probe_raygen(self, params, tables, tiles, n_pool, surplus=128, sentinel=0xC0FFEE5A, check=True):
        """rayn_hip_probe_raygen (rayn_hip.h): k_pack_tables, k_batch_setup and k_raygen on the caller's tables and the tile list `tiles` [n_tiles, 8] uint32.
        -> (rc, dict): geo0, geo1, col0, col1, aov [n_pool + surplus, 4] float32, term_key, term_info, q [n_pool + surplus], pgrp_tile [(n_pool + surplus) / 64],
        tgb, tgc [n_tiles + 2], ctl (dict of the eight words, RAYGEN_CTL), records [(max_bounces + 1) * spp, rec_stride * 4] float32 and records_surplus [64].
        Every array is handed over zeroed, so a refused call leaves zeros.  check=False returns a non-zero rc instead of raising."""
        s1, s2, scr, fis = [np.ascontiguousarray(t, np.float32) for t in tables]
        tiles = np.ascontiguousarray(tiles, np.uint32).reshape(-1, 8)
        n_tiles, NP = tiles.shape[0], n_pool + surplus
        out = {k: np.zeros((NP, 4), np.float32) for k in ("geo0", "geo1", "col0", "col1", "aov")}
        out["term_key"], out["term_info"], out["q"] = np.zeros(NP, np.uint32), np.zeros(NP, np.uint8), np.zeros(NP, np.uint32)
        out["pgrp_tile"], out["tgb"], out["tgc"] = np.zeros(max(NP // 64, 1), np.uint32), np.zeros(n_tiles + 2, np.uint32), np.zeros(n_tiles + 2, np.uint32)
        ctl = np.zeros(8, np.uint32)
        spp, stride = 4 * params.samples, 8 + 12 + 8 * params.volume_marches
        recs = np.zeros((params.max_bounces + 1) * spp * stride + 64, np.float32)
        up, bp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8)))
        rc = self._L.rayn_hip_probe_raygen(self.h, C.byref(params), _fp(s1), s1.size, _fp(s2), s2.size, _fp(scr), scr.size, _fp(fis), n_tiles, up(tiles), n_pool, surplus,
                                           sentinel, *[_fp(out[k]) for k in ("geo0", "geo1", "col0", "col1", "aov")], up(out["term_key"]), bp(out["term_info"]),
                                           up(out["q"]), up(out["pgrp_tile"]), up(out["tgb"]), up(out["tgc"]), up(ctl), _fp(recs))
        if check:
            self._chk(rc)
        out["ctl"] = dict(zip(self.RAYGEN_CTL, ctl.tolist()))
        out["records"], out["records_surplus"] = recs[:-64].reshape(-1, stride), recs[-64:]
        return rc, out

    def probe_shade(self, params, tables, depth, ref, geo0, geo1, col0, col1, max_slots=None, nee_cap=None, sentinel=0xC0FFEE5A, check=True):
        """rayn_hip_probe_shade (rayn_hip.h): the shade stage of one depth on a binned queue `ref` [n_slots] and the pool records geo0 / geo1 / col0 / col1
        [n_pool, 4] float32 in the pool's own encoding.  -> (rc, dict): the pool as the stage left it (geo0, geo1, col0, col1, aov [n_pool, 4], term_key, term_info
        [n_pool]), alive_mask / bgrp_cnt [n_slots / 64], job_count, shadow_jobs, shadow_kernel.  check=False returns a non-zero rc instead of raising."""
        s1, s2, scr, fis = tables
        ref = np.ascontiguousarray(ref, np.uint32)
        recs = [np.ascontiguousarray(a, np.float32).reshape(-1, 4) for a in (geo0, geo1, col0, col1)]
        n_slots, n_pool = ref.size, recs[0].shape[0]
        assert all(a.shape[0] == n_pool for a in recs)
        out = {k: np.zeros((n_pool, 4), np.float32) for k in ("geo0", "geo1", "col0", "col1", "aov")}
        out["term_key"], out["term_info"] = np.zeros(n_pool, np.uint32), np.zeros(n_pool, np.uint8)
        groups = max(n_slots // 64, 1)
        out["alive_mask"], out["bgrp_cnt"] = np.zeros(groups, np.uint64), np.zeros(groups, np.uint8)
        jobs = np.zeros(3, np.uint64)
        up, bp, qp = (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint8))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64)))
        rc = self._L.rayn_hip_probe_shade(self.h, C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), depth, n_slots, n_slots if max_slots is None else max_slots,
                                          n_slots if nee_cap is None else nee_cap, up(ref), n_pool, *[_fp(a) for a in recs], sentinel,
                                          *[_fp(out[k]) for k in ("geo0", "geo1", "col0", "col1", "aov")], up(out["term_key"]), bp(out["term_info"]),
                                          qp(out["alive_mask"]), bp(out["bgrp_cnt"]), qp(jobs))
        if check:
            self._chk(rc)
        out["job_count"], out["shadow_jobs"], out["shadow_kernel"] = int(jobs[0]), int(jobs[1]), ("none", "k_shadow", "k_shadow1", "k_shadow_bulb")[int(jobs[2])]
        return rc, out

    def render_device(self, params, d_tables, d_out, stream=None):
        """rayn_hip_render_frame_device: d_tables/d_out are torch CUDA tensors (kept resident in HBM)."""
        self._chk(self._L.rayn_hip_render_frame_device(self.h, C.byref(params), _ptr(d_tables[0]), _ptr(d_tables[1]), _ptr(d_tables[2]),
                                                       _ptr(d_tables[3]), _ptr(d_out["color"]), _ptr(d_out["alpha"]),
                                                       _ptr(d_out["background"]), _ptr(d_out["normal"]), stream_ptr(stream)))

    def render_packed(self, params, d_tables, d_packed, stream=None):
        """rayn_hip_render_frame_packed_device: the share (params.tile_first / tile_step) straight into its PACKED planar film
        `d_packed` (a float32 CUDA tensor of >= 10 * share_pixels(params) elements) - what a rank hands to the film gather."""
        import torch
        assert d_packed.dtype == torch.float32 and d_packed.is_contiguous() and d_packed.numel() >= 10 * share_pixels(params)
        self._chk(self._L.rayn_hip_render_frame_packed_device(self.h, C.byref(params), _ptr(d_tables[0]), _ptr(d_tables[1]), _ptr(d_tables[2]),
                                                              _ptr(d_tables[3]), _ptr(d_packed), stream_ptr(stream)))

    def unpack_share(self, params, d_packed, d_out, stream=None):
        """rayn_hip_unpack_share_device: scatter the packed film of the share (params.tile_first / tile_step) into the full-resolution
        film `d_out` with one kernel launch on the stream (enqueued, not waited for)."""
        self._chk(self._L.rayn_hip_unpack_share_device(self.h, C.byref(params), _ptr(d_packed), _ptr(d_out["color"]), _ptr(d_out["alpha"]),
                                                       _ptr(d_out["background"]), _ptr(d_out["normal"]), stream_ptr(stream)))

    def save_to_pixels(self, kind, have_mask, transparent_background, width, height, d_film, d_out, stream=None):
        """rayn_hip_save_to_pixels_device: Film::save_to's post-process of channel `kind` (ChannelKind or its value) from the device film
        `d_film` (a dict of torch CUDA tensors as render_device fills them; channels the arm does not read may be absent) into the uint8
        CUDA tensor `d_out` (width * height * bpp bytes, rows top-down).  Enqueued on the stream, not waited for."""
        import torch
        kind = getattr(kind, "value", kind)
        bpp = save_to_bpp(kind, have_mask, transparent_background)
        n = int(width) * int(height)
        if not (d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= n * max(bpp, 0)):
            raise ValueError(f"d_out must be a contiguous uint8 tensor of at least {n * max(bpp, 0)} bytes")
        ptrs = film_ptrs(d_film, FILM_KEYS, n, "d_film")
        self._chk(self._L.rayn_hip_save_to_pixels_device(self.h, int(kind), int(have_mask), int(bool(transparent_background)), int(width), int(height),
                                                         *ptrs, _ptr(d_out), stream_ptr(stream)))

    def png_encode_lz77(self, width, height, bpp, d_img, d_out, d_scratch=None, stream=None):
        """rayn_hip_png_encode_lz77_device: png_encode with LZ77 matches - the same arguments, the same header words and a zlib stream of
        the same filtered rows, smaller on smooth and flat images.  d_scratch: at least png_scratch_bytes_lz77(width, height, bpp) bytes,
        allocated here when None."""
        self.png_encode(width, height, bpp, d_img, d_out, d_scratch, stream, lz77=True)

    def deflate(self, d_data, d_out, stride=0, d_scratch=None, stream=None):
        """rayn_hip_deflate_lz77_device: the zlib stream of the bytes of the contiguous uint8 CUDA tensor `d_data` (1 <= bytes < 2^31)
        into the uint8 CUDA tensor `d_out` (at least deflate_stream_bound(bytes) bytes, 16-byte aligned): the four header words of
        png_encode - the stream's bytes, the input bytes, the blocks, the stored blocks - then the stream, which zlib.decompress takes.
        stride: the distance of the encoder's row candidate, 0 for none.  d_scratch: at least deflate_scratch_bytes(bytes) bytes,
        allocated here when None.  Enqueued on the stream, not waited for; d_data is not modified."""
        import torch
        if d_data is None or not (d_data.dtype == torch.uint8 and d_data.is_contiguous()):
            raise ValueError("d_data must be a contiguous uint8 tensor")
        n = d_data.numel()
        if d_out is None or not (d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= deflate_stream_bound(n)):
            raise ValueError(f"d_out must be a contiguous uint8 tensor of at least {deflate_stream_bound(n)} bytes")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, deflate_scratch_bytes(n), d_out.device)
        self._chk(self._L.rayn_hip_deflate_lz77_device(self.h, _ptr(d_data), n, int(stride), _ptr(d_out), d_out.numel(), scratch_ptr, scratch_bytes,
                                                       stream_ptr(stream)))

    def png_encode(self, width, height, bpp, d_img, d_out, d_scratch=None, stream=None, lz77=False):
        """rayn_hip_png_encode_device: the zlib stream of the PNG IDAT chunk of the 8-bit image `d_img` (a uint8 CUDA tensor of width *
        height * bpp bytes, rows top-down, as save_to_pixels and display write it) into the uint8 CUDA tensor `d_out` (at least
        png_stream_bound(width, height, bpp) bytes, 16-byte aligned): four little-endian words - the stream's bytes, the filtered bytes,
        the blocks, the stored blocks - then the stream (rayn_amd.image.png_from_stream frames it as a file).  d_scratch: a CUDA tensor
        of at least png_scratch_bytes(width, height, bpp) bytes, allocated here when None.  Enqueued on the stream, not waited for; d_img
        is not modified.  lz77: the entry of png_encode_lz77 and its scratch size instead."""
        import torch
        need = int(width) * int(height) * int(bpp)
        for t, label, n in ((d_img, "d_img", need), (d_out, "d_out", png_stream_bound(width, height, bpp))):
            if t is None or not (t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= n):
                raise ValueError(f"{label} must be a contiguous uint8 tensor of at least {n} bytes")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, (png_scratch_bytes_lz77 if lz77 else png_scratch_bytes)(width, height, bpp), d_out.device)
        entry = self._L.rayn_hip_png_encode_lz77_device if lz77 else self._L.rayn_hip_png_encode_device
        self._chk(entry(self.h, int(width), int(height), int(bpp), _ptr(d_img), _ptr(d_out), d_out.numel(), scratch_ptr, scratch_bytes, stream_ptr(stream)))

    def jpeg_encode(self, width, height, bpp, d_img, d_out, quality=90, subsampling=0, restart_interval=JPEG_DEFAULT_RESTART, d_scratch=None, stream=None):
        """rayn_hip_jpeg_encode_device: the entropy-coded scan of the baseline JPEG of the 8-bit image `d_img` (a uint8 CUDA tensor of
        width * height * bpp bytes, bpp 1 or 3, rows top-down, as save_to_pixels and display write it) into the uint8 CUDA tensor `d_out`
        (at least jpeg_scan_bound(width, height, bpp, subsampling, restart_interval) bytes, 16-byte aligned): four little-endian words -
        the scan's bytes, the restart segments, the restart interval, the blocks - then the scan with its RST markers
        (rayn_amd.image.jpeg_from_scan frames it as a file).  quality 1..100; subsampling 0 (4:4:4) or 1 (4:2:0, bpp 3 only);
        restart_interval 1..65535 MCUs.  d_scratch: a CUDA tensor of at least jpeg_scratch_bytes(...) bytes, allocated here when None.
        Enqueued on the stream, not waited for; d_img is not modified."""
        import torch
        need = int(width) * int(height) * int(bpp)
        bound = jpeg_scan_bound(width, height, bpp, subsampling, restart_interval)
        for t, label, n in ((d_img, "d_img", need), (d_out, "d_out", bound)):
            if t is None or not (t.dtype == torch.uint8 and t.is_contiguous() and t.numel() >= n):
                raise ValueError(f"{label} must be a contiguous uint8 tensor of at least {n} bytes")
        a = [int(width), int(height), int(bpp), int(quality), int(subsampling), int(restart_interval)]
        if not all(0 <= v < 1 << 32 for v in a):
            raise ValueError("width, height, bpp, quality, subsampling and restart_interval are unsigned 32-bit values")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, jpeg_scratch_bytes(width, height, bpp, subsampling, restart_interval), d_out.device)
        self._chk(self._L.rayn_hip_jpeg_encode_device(self.h, *a, _ptr(d_img), _ptr(d_out), d_out.numel(), scratch_ptr, scratch_bytes, stream_ptr(stream)))

    def exr_encode(self, width, height, channels, d_out, d_scratch=None, stream=None, lz77=False):
        """rayn_hip_exr_encode_device: the ZIP-compressed scanline chunks of the OpenEXR file of `channels` - a list of (name, tensor,
        stride, offset, type) in the file's order: channel `name` of pixel p (the film's layout, rows bottom-up) is the 32-bit word p *
        stride + offset of the contiguous CUDA tensor of 4-byte elements; type 0 UINT, 1 HALF (the float32 converted), 2 FLOAT - into the
        uint8 CUDA tensor `d_out` (at least exr_stream_bound bytes, 16-byte aligned): four little-endian words - the body's bytes, the
        chunks, the raw chunks, the deflate blocks - the chunk table and the body (rayn_amd.image.exr_from_chunks frames it as a file).
        lz77: the blocks of png_encode_lz77 instead of png_encode's.  d_scratch: at least exr_scratch_bytes bytes, allocated here when
        None.  ValueError for names that are unsorted, duplicated, empty or longer than 31 bytes and for tensors too small.  Enqueued on
        the stream, not waited for; the planes are not modified."""
        import torch
        from . import image
        channels = list(channels)
        image.check_exr_names([c[0] for c in channels])
        width, height = int(width), int(height)
        layout = [(int(s), int(o), int(t)) for _, _, s, o, t in channels]
        bound = exr_stream_bound(width, height, layout)
        for name, t, s, o, _ in channels:
            need = (width * height - 1) * int(s) + int(o) + 1
            if t is None or not (t.is_cuda and t.element_size() == 4 and t.is_contiguous() and t.numel() >= need):
                raise ValueError(f"channel {name!r} must be a contiguous CUDA tensor of at least {need} 32-bit elements")
        if d_out is None or not (d_out.dtype == torch.uint8 and d_out.is_contiguous() and d_out.numel() >= max(bound, 1)):
            raise ValueError(f"d_out must be a contiguous uint8 tensor of at least {bound} bytes")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, exr_scratch_bytes(width, height, layout, lz77), d_out.device)
        n, words = _exr_layout(layout)
        planes = (C.c_void_p * max(n, 1))(*[t.data_ptr() for _, t, _, _, _ in channels])
        self._chk(self._L.rayn_hip_exr_encode_device(self.h, width, height, n, planes, words, int(bool(lz77)), _ptr(d_out), d_out.numel(), scratch_ptr,
                                                     scratch_bytes, stream_ptr(stream)))

    def display_state(self):
        """A fresh state of the display transform's auto exposure: two zeroed 32-bit words {m, valid} on the context's GPU."""
        import torch
        return torch.zeros(2, dtype=torch.int32, device=f"cuda:{self.device}")

    def display(self, display, have_mask, transparent_background, width, height, d_film, d_out, d_state=None, d_scratch=None, adapt=1.0,
                d_out_meter=None, d_out_bloom=None, stream=None):
        """rayn_hip_display_pixels_device / rayn_hip_display_color_device: the HDR display transform (Display `display`) of the Color kind
        of the device film `d_film` (as save_to_pixels takes it).  A uint8 `d_out` (width * height * bpp bytes) receives the 8-bit image,
        rows top-down; a float32 one (width * height * 3 floats) the float plane before gamma and quantisation, in film order.  d_state
        (display_state(); auto exposure only) carries the metered value between calls, blended with weight `adapt`; None = a fresh one.
        d_scratch: a CUDA tensor of at least display_scratch_bytes(width, height, display.levels) bytes, allocated here when None and
        needed.  d_out_meter (2 floats: m, e) and d_out_bloom (width * height * 3 floats) are optional float32 outputs.  Enqueued on the
        stream, not waited for; the exposure never comes to the host."""
        import torch
        n = int(width) * int(height)
        bpp = save_to_bpp(0, have_mask, transparent_background)
        if d_out.dtype == torch.uint8:
            fn, need = self._L.rayn_hip_display_pixels_device, n * max(bpp, 0)
        elif d_out.dtype == torch.float32:
            fn, need = self._L.rayn_hip_display_color_device, 3 * n
        else:
            raise ValueError("d_out must be a uint8 tensor (the image) or a float32 tensor (the float plane)")
        if not (d_out.is_contiguous() and d_out.numel() >= need):
            raise ValueError(f"d_out must be contiguous and hold at least {need} elements")
        meter, bloom = opt_f32_ptr(d_out_meter, "d_out_meter", 2), opt_f32_ptr(d_out_bloom, "d_out_bloom", 3 * n)
        ptrs = film_ptrs(d_film, FILM_KEYS[:3], n, "d_film")
        if display.auto and d_state is None:
            d_state = torch.zeros(2, dtype=torch.int32, device=d_out.device)
        if d_state is not None and not (d_state.dtype == torch.int32 and d_state.is_contiguous() and d_state.numel() >= 2):
            raise ValueError("d_state must be a contiguous int32 tensor of 2 elements (Context.display_state())")
        scratch_ptr, scratch_bytes = None, 0  # a manual exposure without bloom needs none
        if d_scratch is not None or display.auto or display.levels:
            d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, display_scratch_bytes(width, height, display.levels), d_out.device)
        dp = display.to_abi(adapt)
        self._chk(fn(self.h, C.byref(dp), int(have_mask), int(bool(transparent_background)), int(width), int(height), *ptrs, _opt_ptr(d_state),
                     scratch_ptr, scratch_bytes, _ptr(d_out), meter, bloom, stream_ptr(stream)))

    def upscale(self, params, upscale, d_film, d_low_gbuffer, d_high_gbuffer, d_out_film, d_out_weight=None, stream=None):
        """rayn_hip_upscale_device: the guided upscaling (Upscale `upscale`) of the device film `d_film` of the frame `params` (its width
        and height are the LOW film's) into `d_out_film`, a film dict of upscale.factor times that size.  d_low_gbuffer / d_high_gbuffer:
        the G-buffers (alloc_gbuffer's dicts, as Context.gbuffer fills them) of the frame at the low and at the high resolution.  A plane
        (alpha, background, normal) the film lacks is absent from d_film and d_out_film together and is neither read nor written; "color"
        is required.  d_out_weight: a float32 CUDA tensor of one float per high pixel for the summed guided weight (0 where a fallback
        was taken), or None.  Enqueued on the stream, not waited for."""
        low, gp, high, weight = _upscale_args(params, upscale, d_film, d_low_gbuffer, d_high_gbuffer, d_out_film, d_out_weight)
        up = upscale.to_abi()
        self._chk(self._L.rayn_hip_upscale_device(self.h, int(params.width), int(params.height), C.byref(up), *low, *gp, *high, weight,
                                                  stream_ptr(stream)))

    def temporal_upscale(self, params, upscale, temporal, supersample, d_film, d_low_gbuffer, d_high_gbuffer, d_prev_history, prev_camera,
                         prev_time_start, d_new_history, d_out_film, low_camera=None, d_out_weight=None, stream=None):
        """rayn_hip_temporal_upscale_device: the guided upscaling (Upscale `upscale`) of the low device film `d_film` of the frame `params`
        (its width and height are the LOW film's) fused with the temporal accumulation (Temporal `temporal`; its resample and feedback are
        not part of this entry) at upscale.factor times that size, by the Supersample `supersample`.  d_low_gbuffer / d_high_gbuffer: the
        frame's G-buffers at both resolutions, the low one traced through `low_camera` (an _abi.Camera: the camera the low film was
        rendered with, or None for the frame's own - the default footprint), the high one through the frame's own camera.
        d_prev_history / d_new_history: uint8 CUDA tensors of temporal_history_bytes at the HIGH size (d_prev_history None: no history),
        reprojected through prev_camera at prev_time_start.  d_out_film: a film dict of the high size; "color" receives the ACCUMULATED
        colour, "alpha" / "background" (absent together with d_film's) and "normal" this frame's upscaled planes.  "color" and "normal"
        are required on both sides.  d_out_weight: a float32 CUDA tensor of one float per high pixel, or None.  Enqueued on the stream, not
        waited for."""
        low, gp, high, weight = _upscale_args(params, upscale, d_film, d_low_gbuffer, d_high_gbuffer, d_out_film, d_out_weight)
        prev, new, nbytes = byte_ptrs(d_new_history, "d_new_history", d_prev_history, "d_prev_history")
        up, tp, sp = upscale.to_abi(), temporal.to_abi(), supersample.to_abi()
        self._chk(self._L.rayn_hip_temporal_upscale_device(
            self.h, C.byref(params), C.byref(up), C.byref(tp), C.byref(sp), None if low_camera is None else C.byref(low_camera),
            None if prev_camera is None else C.byref(prev_camera), float(prev_time_start), *low, *gp, prev, new, nbytes, *high, weight,
            stream_ptr(stream)))

    def denoise(self, width, height, d_film, d_out_color, params, d_scratch=None, stream=None):
        """rayn_hip_denoise_device: the a-trous denoiser (Denoise `params`) of d_film["color"] into the float32 CUDA tensor d_out_color
        (width * height * 3 floats), guided by d_film["normal"] and d_film["alpha"] (a guide whose sigma is 0 may be absent).
        d_scratch: a CUDA tensor of at least denoise_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the
        stream, not waited for."""
        n = int(width) * int(height)
        out = f32_ptr(d_out_color, "d_out_color", 3 * n)
        ptrs = film_ptrs(d_film, GUIDE_KEYS, n, "d_film")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, denoise_scratch_bytes(width, height), d_out_color.device)
        self._chk(self._L.rayn_hip_denoise_device(self.h, int(width), int(height), int(params.iterations), float(params.sigma_color),
                                                  float(params.sigma_normal), float(params.sigma_alpha), *ptrs, out, scratch_ptr, scratch_bytes,
                                                  stream_ptr(stream)))

    def denoise_variance(self, params, d_film, d_state, d_out_color, denoise, d_out_variance=None, d_scratch=None, stream=None):
        """rayn_hip_denoise_variance_device: the variance-guided a-trous denoiser (VarianceDenoise `denoise`) of the mean film
        d_film["color"] of a progressive render into the float32 CUDA tensor d_out_color (width * height * 3 floats), guided by
        d_film["normal"] and d_film["alpha"] (a guide whose sigma is 0 may be absent) and by the render's state `d_state` with the film
        geometry of `params` (as progressive_accumulate takes them).  d_out_variance: a float32 CUDA tensor of width * height floats for
        the filtered variance, or None.  d_scratch: a CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes,
        allocated here when None.  Enqueued on the stream, not waited for."""
        width, height = params.width, params.height
        n = int(width) * int(height)
        out, var = f32_ptr(d_out_color, "d_out_color", 3 * n), opt_f32_ptr(d_out_variance, "d_out_variance", n)
        ptrs = film_ptrs(d_film, GUIDE_KEYS, n, "d_film")
        state_ptr, state_bytes = self._prog_state(params, d_state)
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, denoise_variance_scratch_bytes(width, height), d_out_color.device)
        self._chk(self._L.rayn_hip_denoise_variance_device(self.h, C.byref(params), int(denoise.iterations), float(denoise.sigma_luminance),
                                                           float(denoise.sigma_normal), float(denoise.sigma_alpha), *ptrs, state_ptr, state_bytes,
                                                           out, var, scratch_ptr, scratch_bytes, stream_ptr(stream)))

    def gbuffer(self, params, d_gbuffer, d_scratch=None, stream=None):
        """rayn_hip_gbuffer_device: the primary-hit G-buffer of the uploaded world under `params` (resolution, time_start, march constants)
        into d_gbuffer (alloc_gbuffer's dict: "records" (n, 4) float32 = (Px, Py, Pz, t), "object" (n,) int32).  d_scratch: a CUDA tensor
        of at least gbuffer_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the stream, not waited for."""
        rec, obj = gbuffer_ptrs(d_gbuffer, int(params.width) * int(params.height), "d_gbuffer")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, gbuffer_scratch_bytes(params.width, params.height), d_gbuffer["records"].device)
        self._chk(self._L.rayn_hip_gbuffer_device(self.h, C.byref(params), rec, obj, scratch_ptr, scratch_bytes, stream_ptr(stream)))

    def preview(self, params, preview, d_samples, d_out_film, d_scramble=None, d_out_ao=None, d_out_gbuffer=None, d_scratch=None, stream=None):
        """rayn_hip_preview_device: the preview integrator (Preview `preview`) of the uploaded world under `params` (resolution, time_start,
        march constants): primary hit, viewer-facing normal and ambient occlusion.  d_samples: a float32 CUDA tensor of 2 * preview.samples
        floats, the AO sample pairs; d_scramble: one float per pixel, or None for none (preview_tables builds the defaults of both).
        d_out_film: a film dict whose "color", "alpha" and "normal" planes are written (a "background" plane is not touched: the preview
        has none).  d_out_ao: a float32 CUDA tensor of one float per pixel, or None.  d_out_gbuffer: alloc_gbuffer's dict for the primary
        hits - bit for bit what Context.gbuffer writes - or None.  d_scratch: a CUDA tensor of at least preview_scratch_bytes(width,
        height, preview.samples) bytes, allocated here when None.  Enqueued on the stream, not waited for."""
        n = int(params.width) * int(params.height)
        smp = f32_ptr(d_samples, "d_samples", 2 * int(preview.samples))
        scr, ao = opt_f32_ptr(d_scramble, "d_scramble", n), opt_f32_ptr(d_out_ao, "d_out_ao", n)
        out = [f32_ptr(d_out_film.get(k), f"d_out_film[{k!r}]", _PLANE_FLOATS[k] * n) for k in ("color", "alpha", "normal")]
        rec, obj = (None, None) if d_out_gbuffer is None else gbuffer_ptrs(d_out_gbuffer, n, "d_out_gbuffer")
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, preview_scratch_bytes(params.width, params.height, preview.samples),
                                                        d_out_film["color"].device)
        pp = preview.to_abi()
        self._chk(self._L.rayn_hip_preview_device(self.h, C.byref(params), C.byref(pp), smp, scr, *out, ao, rec, obj, scratch_ptr, scratch_bytes,
                                                  stream_ptr(stream)))

    def interpolate(self, params, interpolate, key_a, key_b, d_gbuffer, d_out_film, d_out_source=None, stream=None):
        """rayn_hip_interpolate_device: the film planes of the frame `params` (its width, height and time_start) generated from two rendered
        key frames by the Interpolate `interpolate`.  A key is (film dict, G-buffer dict, _abi.Camera, time_start): the device film of the key,
        its G-buffer (alloc_gbuffer's dict, as Context.gbuffer fills it at the key's time_start), the camera it was rendered through and
        its time_start; key_a lies before key_b and params.time_start between them.  d_gbuffer: the frame's own G-buffer under the same
        uploaded world.  d_out_film: a film dict of the same size.  A plane (alpha, background, normal) the films lack is absent from both
        keys and d_out_film together and is neither read nor written; "color" is required.  d_out_source: an int32 CUDA tensor of one
        element per pixel for the arm that produced the pixel (0 both keys, 1 A only, 2 B only, 3 cross-fade, 4 a single key's pixel), or
        None.  Enqueued on the stream, not waited for."""
        n = int(params.width) * int(params.height)
        keys, cams = [], []
        for label, key in (("key_a", key_a), ("key_b", key_b)):
            film, gbuf, camera, time_start = key
            if not isinstance(camera, _abi.Camera):
                raise ValueError(f"{label}'s camera must be an _abi.Camera")
            planes = film_ptrs(film, FILM_KEYS, n, f"{label}'s film")
            if planes[0] is None:
                raise ValueError(f"{label}'s film['color'] must be a contiguous float32 tensor of at least {3 * n} floats")
            rec, obj = gbuffer_ptrs(gbuf, n, f"{label}'s G-buffer")
            cams.append(camera)  # held until the call returns: the key points at it
            keys.append(_abi.InterpolateKey(*[None if q is None else q.value for q in planes], rec.value, obj.value, C.addressof(camera),
                                            float(time_start)))
        rec, obj = gbuffer_ptrs(d_gbuffer, n, "d_gbuffer")
        out = film_ptrs(d_out_film, FILM_KEYS, n, "d_out_film")
        src = None if d_out_source is None else i32_ptr(d_out_source, "d_out_source", n)
        ip = interpolate.to_abi()
        self._chk(self._L.rayn_hip_interpolate_device(self.h, C.byref(params), C.byref(ip), C.byref(keys[0]), C.byref(keys[1]), rec, obj, *out, src,
                                                      stream_ptr(stream)))

    def temporal_accumulate(self, params, temporal, d_film, d_gbuffer, d_prev_history, prev_camera, prev_time_start, d_new_history, d_out_color,
                            stream=None, d_prev_moments=None, d_new_moments=None):
        """rayn_hip_temporal_accumulate_device: blend d_film["color"] (guides: d_film["normal"], the G-buffer d_gbuffer of the same frame)
        with the previous frame's history d_prev_history (a uint8 CUDA tensor of temporal_history_bytes, or None: no history) reprojected
        through prev_camera (an _abi.Camera) at prev_time_start, by the Temporal `temporal`.  Writes the accumulated colour to the float32
        CUDA tensor d_out_color (width * height * 3 floats) and the new history to d_new_history.  Enqueued on the stream, not waited for.

        With d_new_moments (a uint8 CUDA tensor of temporal_moments_bytes; d_prev_moments beside d_prev_history, None with it) the call
        goes through rayn_hip_temporal_accumulate_moments_device, which also carries the first and second moment of the luminance through
        the same reprojection - what denoise_temporal_variance reads; colour and history are the same bits.  Both None: the plain entry.

        temporal.resample == "bilinear" calls these two entries; "catmull_rom" goes through rayn_hip_temporal_accumulate_resample_device
        instead, with or without moments, under the same rules."""
        n = int(params.width) * int(params.height)
        planes = [f32_ptr(d_film.get("color"), "'color'", 3 * n), f32_ptr(d_film.get("normal"), "'normal'", 3 * n),
                  f32_ptr(d_gbuffer.get("records"), "'records'", 4 * n), i32_ptr(d_gbuffer.get("object"), "d_gbuffer['object']", n)]
        out = f32_ptr(d_out_color, "d_out_color", 3 * n)
        history = byte_ptrs(d_new_history, "d_new_history", d_prev_history, "d_prev_history")
        moments = (None, None, 0)
        if d_prev_moments is not None or d_new_moments is not None:
            moments = byte_ptrs(d_new_moments, "d_new_moments", d_prev_moments, "d_prev_moments")
        tp = temporal.to_abi()
        head = (self.h, C.byref(params), C.byref(tp))
        tail = (None if prev_camera is None else C.byref(prev_camera), float(prev_time_start), *planes, *history)
        if temporal.resample != "bilinear":  # this entry takes the moments or their absence
            rp = temporal.resample_to_abi()
            rc = self._L.rayn_hip_temporal_accumulate_resample_device(*head, C.byref(rp), *tail, *moments, out, stream_ptr(stream))
        elif moments[1] is not None:
            rc = self._L.rayn_hip_temporal_accumulate_moments_device(*head, *tail, *moments, out, stream_ptr(stream))
        else:
            rc = self._L.rayn_hip_temporal_accumulate_device(*head, *tail, out, stream_ptr(stream))
        self._chk(rc)

    def denoise_temporal_variance(self, width, height, d_film, d_gbuffer, d_history, d_moments, d_out_color, denoise, d_out_variance=None,
                                  d_scratch=None, stream=None, feedback=0.0):
        """rayn_hip_denoise_temporal_variance_device: the variance-guided a-trous denoiser (VarianceDenoise `denoise`) of a temporally
        accumulated colour.  d_film["color"] is the ACCUMULATED colour (what temporal_accumulate wrote to d_out_color), d_film["normal"] /
        d_film["alpha"] the film's guides (a guide whose sigma is 0 may be absent), d_gbuffer the frame's G-buffer (its "object" plane is
        read), d_history / d_moments the NEW history and moments of that accumulate.  A pixel's variance comes from its moments once its
        history is 4 frames long, (m2 - m1^2) / n, and from the 7x7 neighbourhood of the accumulated luminance on the same object before
        that - so with Temporal(max_history < 4) only the spatial estimate is ever used.  Writes the float32 CUDA tensor d_out_color
        (width * height * 3 floats) and, when given, d_out_variance (width * height floats; NaN where there was no estimate).  d_scratch: a
        CUDA tensor of at least denoise_variance_scratch_bytes(width, height) bytes, allocated here when None.  Enqueued on the stream,
        not waited for.  Recommended for sequences: VarianceDenoise(1, 4.0, 0.4, 0.3), 0.46x the raw frame where Temporal() alone gives 0.49x.

        feedback (finite, in [0, 1]): 0 takes the entry above and leaves d_history alone.  Anything else goes through
        rayn_hip_denoise_temporal_variance_feedback_device: d_out_color and d_out_variance are the same bits, and the colour of d_history
        becomes c + feedback * (c' - c), c' the output of the first a-trous pass, wherever that pass had an estimate; the history lengths,
        the other planes of the history and the moments are not written."""
        feedback = float(feedback)
        if not 0.0 <= feedback <= 1.0:
            raise ValueError(f"feedback must be finite and in [0, 1], got {feedback!r}")
        n = int(width) * int(height)
        out, var = f32_ptr(d_out_color, "d_out_color", 3 * n), opt_f32_ptr(d_out_variance, "d_out_variance", n)
        ptrs = film_ptrs(d_film, GUIDE_KEYS, n, "d_film")
        obj = i32_ptr(d_gbuffer.get("object"), "d_gbuffer['object']", n)
        history, moments = byte_ptrs(d_history, "d_history")[1:], byte_ptrs(d_moments, "d_moments")[1:]
        d_scratch, scratch_ptr, scratch_bytes = scratch(d_scratch, denoise_variance_scratch_bytes(width, height), d_out_color.device)
        args = (self.h, int(width), int(height), int(denoise.iterations), float(denoise.sigma_luminance), float(denoise.sigma_normal),
                float(denoise.sigma_alpha), *ptrs, obj, *history, *moments, out, var, scratch_ptr, scratch_bytes)
        if feedback == 0.0:
            self._chk(self._L.rayn_hip_denoise_temporal_variance_device(*args, stream_ptr(stream)))
        else:
            self._chk(self._L.rayn_hip_denoise_temporal_variance_feedback_device(*args, feedback, stream_ptr(stream)))

    @staticmethod
    def _prog_state(params, d_state):
        need = _prog.state_bytes(params.width, params.height, (params.tile_w, params.tile_h))
        _, ptr, nbytes = byte_ptrs(d_state, "d_state")
        if need and nbytes < need:
            raise ValueError(f"d_state must hold at least {need} bytes")
        return ptr, nbytes

    def progressive_reset(self, params, d_state, stream=None):
        """rayn_hip_progressive_reset_device: a fresh progressive state for the film geometry of `params` in the uint8 CUDA tensor
        `d_state` (at least rayn_amd.progressive.state_bytes).  Enqueued on the stream, not waited for."""
        ptr, nbytes = self._prog_state(params, d_state)
        self._chk(self._L.rayn_hip_progressive_reset_device(self.h, C.byref(params), ptr, nbytes, stream_ptr(stream)))

    def progressive_accumulate(self, params, progressive, tiles, d_epoch, d_state, d_mean, stream=None):
        """rayn_hip_progressive_accumulate_device: accumulate the epoch film `d_epoch` (a dict of torch CUDA tensors as render_device
        fills them) into the tiles `tiles` (ascending indices; None = every tile) of `d_state`, write those tiles' mean film to `d_mean`,
        retire tiles by the Progressive `progressive` and compact the active list.  Enqueued on the stream, not waited for."""
        n = params.width * params.height
        epoch, mean = ([f32_ptr(film.get(k), f"film[{k!r}]", _PLANE_FLOATS[k] * n) for k in FILM_KEYS] for film in (d_epoch, d_mean))
        ptr, nbytes = self._prog_state(params, d_state)
        arr, n_tiles = None, 0
        if tiles is not None:
            arr = np.ascontiguousarray(tiles, dtype=np.uint32)
            n_tiles = len(arr)
        pp = progressive.to_abi()
        self._chk(self._L.rayn_hip_progressive_accumulate_device(self.h, C.byref(params), C.byref(pp),
                                                                 None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles,
                                                                 *epoch, ptr, nbytes, *mean, stream_ptr(stream)))

    def progressive_fetch_active(self, params, d_state, stream=None):
        """rayn_hip_progressive_fetch_active (blocking): (the ascending list of the tiles not retired as a uint32 array, totals dict)."""
        ptr, nbytes = self._prog_state(params, d_state)
        cap = int(self._L.rayn_tile_count(params.width, params.height, params.tile_w, params.tile_h))
        out = np.zeros(max(cap, 1), np.uint32)
        tot = _abi.ProgressiveTotals()
        n = self._L.rayn_hip_progressive_fetch_active(self.h, C.byref(params), ptr, nbytes, out.ctypes.data_as(C.POINTER(C.c_uint32)), cap,
                                                      C.byref(tot), stream_ptr(stream))
        if n < 0:
            self._chk(int(n))
        return out[:n].copy(), {"active_tiles": int(tot.active_tiles), "max_e": float(tot.max_e), "outlier_pixels": int(tot.outlier_pixels)}

    def progressive_tile_report(self, params, d_state, stream=None):
        """rayn_hip_progressive_tile_report (blocking): dict of per-tile arrays epochs, retired, outliers (uint32) and max_e (float32)."""
        ptr, nbytes = self._prog_state(params, d_state)
        t = max(int(self._L.rayn_tile_count(params.width, params.height, params.tile_w, params.tile_h)), 1)
        rep = {"epochs": np.zeros(t, np.uint32), "retired": np.zeros(t, np.uint32), "outliers": np.zeros(t, np.uint32), "max_e": np.zeros(t, np.float32)}
        up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        self._chk(self._L.rayn_hip_progressive_tile_report(self.h, C.byref(params), ptr, nbytes, up(rep["epochs"]), up(rep["retired"]),
                                                           up(rep["outliers"]), _fp(rep["max_e"]), stream_ptr(stream)))
        return rep

    def close(self):
        if self.h:
            self._L.rayn_hip_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def save_to_bpp(kind, have_mask, transparent_background=False):
    """rayn_save_to_bpp: bytes per pixel of the image Film::save_to writes for channel `kind` given the film's channels (bit k of
    have_mask = ChannelKind k), or -1 where the reference returns Err.  Host only."""
    return int(lib().rayn_save_to_bpp(int(getattr(kind, "value", kind)), int(have_mask), int(bool(transparent_background))))


def alloc_device_film(width, height, device="cuda"):
    import torch
    n = width * height
    return {"color": torch.zeros(n, 3, dtype=torch.float32, device=device), "alpha": torch.zeros(n, dtype=torch.float32, device=device),
            "background": torch.zeros(n, 3, dtype=torch.float32, device=device), "normal": torch.zeros(n, 3, dtype=torch.float32, device=device)}
