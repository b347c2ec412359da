"""ctypes binding of the CPU oracle (oracle/librayn_oracle.so).

TEST INFRASTRUCTURE: imported only by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  The product package (rayn_amd/) never imports this module."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))


# oracle_counters::tally / the out_tally of oracle_shade_packets_counts: the PER-LANE accounting the HIP path's instrumented kernels are held to
TALLY_KEYS = ("evals_extend", "evals_shade_setup", "evals_shadow", "iters_extend", "iters_shade_setup", "iters_shadow",
              "zero_throughput_slots", "elided_shadow_jobs", "samples_out_of_bounds", "shadow_jobs", "sphere_blocked_samples", "jobs_first_sdf_occludes", "jobs_all_sdfs_marched")


class Counters(C.Structure):
    """dist_evals counts four lanes per packet call; tally (TALLY_KEYS) counts per lane: a lane is charged while it holds a ray and has not stopped."""
    _fields_ = [("paths", C.c_uint64), ("segments", C.c_uint64), ("packets", C.c_uint64),
                ("dist_evals", C.c_uint64), ("tiles", C.c_uint64), ("tally", C.c_uint64 * 13)]

    def lane_counts(self):
        """The per-lane accounting of the frame as a dict over TALLY_KEYS."""
        return {k: int(v) for k, v in zip(TALLY_KEYS, self.tally)}

    def device_counts(self):
        """What a counting HIP context reports for the same frame: (eval_counts, sdf_iterations, elision_counts, shadow_jobs)."""
        t = [int(v) for v in self.tally]
        return t[0:3], t[3:6], t[6:9], t[9]


def build(force=False):
    """Compile the oracle with g++ (oracle/Makefile)."""
    if force:
        subprocess.check_call(["make", "-C", _HERE, "clean"], stdout=subprocess.DEVNULL)
    subprocess.check_call(["make", "-C", _HERE, "-j2"], stdout=subprocess.DEVNULL)


_libs = {}


VARIANTS = ("minmax_swapped", "minmax_ieee", "libm", "normalize_div", "dot_plain", "normals_central", "normals_order", "lerp_alt")


def build_variants():
    """The alternative-reading libraries of oracle/Makefile `variants` (oracle/SENSITIVITY.md); never used by the parity tests."""
    subprocess.check_call(["make", "-C", _HERE, "-j4", "variants"], stdout=subprocess.DEVNULL)


def lib(fma=False, variant=None):
    """The oracle library: default (unfused mul_add), fma=True (fused), or variant=<name of VARIANTS> = ONE assumption of the
    header's list read the other way (sensitivity analysis / naming a wrong assumption when pinning against rayn)."""
    if variant is not None:
        assert variant in VARIANTS and not fma, variant
    name = f"librayn_oracle_{variant}.so" if variant else ("librayn_oracle_fma.so" if fma else "librayn_oracle.so")
    if name not in _libs:
        path = os.path.join(_HERE, name)
        if variant:
            build_variants()  # through make every time: a variant library left from older sources lacks the entries bound below
        elif not os.path.exists(path):
            build()
        L = C.CDLL(path)
        fp = C.POINTER(C.c_float)
        up = C.POINTER(C.c_uint32)
        L.oracle_sets_1d.restype = C.c_uint32
        L.oracle_sets_2d.restype = C.c_uint32
        L.oracle_tile_count.restype = C.c_uint32
        L.oracle_render_frame.restype = C.c_int
        L.oracle_render_frame.argtypes = [C.c_void_p, C.c_void_p, fp, fp, fp, fp, fp, fp, fp, fp, C.c_int, up,
                                          C.c_uint32, C.POINTER(Counters)]
        L.oracle_trace_tile.restype = C.c_int64
        L.oracle_trace_tile.argtypes = [C.c_void_p, C.c_void_p, fp, fp, fp, fp, C.c_uint32, C.c_uint64,
                                        up, up, up, up, up, up]
        L.oracle_trace_shade.restype = C.c_int64
        L.oracle_trace_shade.argtypes = [C.c_void_p, C.c_void_p, fp, fp, fp, fp, C.c_uint32, C.c_uint64, up, up, fp, up, fp]
        L.oracle_raygen_tile.restype = C.c_int64
        L.oracle_raygen_tile.argtypes = [C.c_void_p, C.c_void_p, fp, fp, fp, fp] + [C.c_uint32] * 4 + [C.c_uint64, fp, up]
        L.oracle_shade_packets.restype = C.c_int
        L.oracle_shade_packets.argtypes = [C.c_void_p, C.c_void_p, fp, fp, C.c_uint32, C.c_uint64, up, up, fp, up, fp]
        u64p = C.POINTER(C.c_uint64)
        L.oracle_shade_packets_counts.restype = C.c_int
        L.oracle_shade_packets_counts.argtypes = [C.c_void_p, C.c_void_p, fp, fp, C.c_uint32, C.c_uint64, up, up, fp, up, fp, u64p]
        L.oracle_closest_hit_counts.restype = None
        L.oracle_closest_hit_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, fp, fp, fp, up, up, up, C.c_uint64]
        L.oracle_shadow_counts.restype = None
        L.oracle_shadow_counts.argtypes = [C.c_void_p, C.c_void_p, fp, fp, fp, up, up, C.c_uint64]
        L.oracle_set_job_sink.restype = None
        L.oracle_set_job_sink.argtypes = [C.c_int]
        L.oracle_take_job_sink.restype = C.c_uint64
        L.oracle_take_job_sink.argtypes = [fp, C.c_uint64]
        L.oracle_sdf_steps.restype = None
        L.oracle_sdf_steps.argtypes = [C.c_void_p, fp, up, C.c_uint64]
        L.oracle_build_rd_tables.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, fp, fp]
        L.oracle_build_scramble.argtypes = [C.c_uint32, C.c_uint32, fp]
        L.oracle_build_fis_table.argtypes = [C.c_uint32, C.c_float, fp]
        L.oracle_build_fis_table_ex.argtypes = [C.c_uint32, C.c_float, C.c_float, C.c_float, fp]
        _libs[name] = L
    return _libs[name]


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def build_tables(spp, max_bounces, volume_marches, frame, width, height, filter_kind=0, filter_radius=1.5, fma=False, filter_params=(0.0, 0.0), variant=None):
    """Samples::new_rd + per-pixel scramble + FilterImportanceSampler::new, oracle versions."""
    L = lib(fma, variant)
    n1 = L.oracle_sets_1d(max_bounces, volume_marches)
    n2 = L.oracle_sets_2d(max_bounces, volume_marches)
    s1 = np.zeros(spp * n1, np.float32)
    s2 = np.zeros(spp * 2 * n2, np.float32)
    L.oracle_build_rd_tables(spp, n1, n2, frame, _fp(s1), _fp(s2))
    scr = np.zeros(width * height, np.float32)
    L.oracle_build_scramble(width, height, _fp(scr))
    fis = np.zeros(512, np.float32)
    L.oracle_build_fis_table_ex(filter_kind, filter_radius, filter_params[0], filter_params[1], _fp(fis))
    return s1, s2, scr, fis


def render(world_desc, params, tables, threads=None, tile_subset=None, fma=False, variant=None):
    """Film::render_frame_into on the CPU.  Returns (film dict, Counters)."""
    L = lib(fma, variant)
    s1, s2, scr, fis = tables
    n = params.width * params.height
    color = np.zeros((n, 3), np.float32)
    alpha = np.zeros(n, np.float32)
    bg = np.zeros((n, 3), np.float32)
    normal = np.zeros((n, 3), np.float32)
    ctr = Counters()
    if threads is None:
        threads = os.cpu_count() or 1
    sub, nsub = None, 0
    if tile_subset is not None:
        arr = np.ascontiguousarray(tile_subset, dtype=np.uint32)
        sub, nsub = _up(arr), len(arr)
    rc = L.oracle_render_frame(C.byref(world_desc), C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis),
                               _fp(color), _fp(alpha), _fp(bg), _fp(normal), threads, sub, nsub, C.byref(ctr))
    if rc != 0:
        raise RuntimeError(f"oracle_render_frame failed: {rc}")
    h, w = params.height, params.width
    return {"color": color.reshape(h, w, 3), "alpha": alpha.reshape(h, w), "background": bg.reshape(h, w, 3),
            "normal": normal.reshape(h, w, 3)}, ctr


def trace_tile(world_desc, params, tables, tile_index, fma=False, variant=None):
    """Per-depth packet lanes of one tile in process_hits order: dict of uint32 arrays."""
    L = lib(fma, variant)
    s1, s2, scr, fis = tables
    cap = (params.tile_w * params.tile_h * params.samples * 4 + 64) * (params.max_bounces + 2)
    arrs = [np.zeros(cap, np.uint32) for _ in range(6)]
    n = L.oracle_trace_tile(C.byref(world_desc), C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), tile_index,
                            cap, *[_up(a) for a in arrs])
    if n < 0 or n > cap:
        raise RuntimeError(f"oracle_trace_tile failed: {n}")
    keys = ["depth", "obj", "px", "py", "sample", "valid"]
    return {k: a[:n].copy() for k, a in zip(keys, arrs)}


def raygen_tile(world_desc, params, tables, x0, y0, x1, y1, fma=False):
    """The ray-gen loop of the tile [x0, x1) x [y0, y1) (any rectangle inside the film), through the function the film's tile closure calls.  dict over the
    paths in the reference's order (x outer, y inner, packet, lane): origin, dir [n, 3], time [n] float32; pixel (x + y * width), sample [n] uint32."""
    L = lib(fma)
    s1, s2, scr, fis = [np.ascontiguousarray(t, np.float32) for t in tables]
    assert scr.size == params.width * params.height and fis.size == 512
    cap = max(int(x1) - int(x0), 0) * max(int(y1) - int(y0), 0) * params.samples * 4
    f, u = np.zeros((max(cap, 1), 7), np.float32), np.zeros((max(cap, 1), 2), np.uint32)
    n = L.oracle_raygen_tile(C.byref(world_desc), C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), x0, y0, x1, y1, cap, _fp(f), _up(u))
    if n != cap or n <= 0:
        raise ValueError(f"oracle_raygen_tile failed: {n}")
    return {"origin": f[:, 0:3].copy(), "dir": f[:, 3:6].copy(), "time": f[:, 6].copy(), "pixel": u[:, 0].copy(), "sample": u[:, 1].copy()}


# lane status of shade_packets / trace_shade
SH_INVALID, SH_SPAWNED, SH_COLOR, SH_BACKGROUND = 0, 1, 2, 3
# the 15 floats of a lane: what goes in ...
SHADE_IN = {"origin": slice(0, 3), "dir": slice(3, 6), "t": 6, "time": 7, "radiance": slice(8, 11), "throughput": slice(11, 14), "scramble": 14}
# ... and what comes out (what the status does not define is 0: a terminated lane has only its radiance, the Color / Background sample)
SHADE_OUT = {"radiance": slice(0, 3), "throughput": slice(3, 6), "origin": slice(6, 9), "dir": slice(9, 12), "normal": slice(12, 15)}


def _shade_dict(pk, lane_u, lane_f, out_u, out_f):
    return {"depth": pk[:, 0].copy(), "obj": pk[:, 1].copy(), "valid": lane_u[:, :, 0].copy(), "sample": lane_u[:, :, 1].copy(), "tcx": lane_u[:, :, 2].copy(),
            "tcy": lane_u[:, :, 3].copy(), "lane_f": lane_f, "status": out_u[:, :, 0].copy(), "aov": out_u[:, :, 1].copy(), "out_f": out_f}


def trace_shade(world_desc, params, tables, tile_index, fma=False):
    """Every Integrator::integrate call of one tile, rendered single-threaded, per depth in process_hits order.  dict of arrays over the n packets:
    depth, obj [n]; valid, sample, tcx, tcy [n, 4]; lane_f [n, 4, 15] (SHADE_IN); status, aov [n, 4]; out_f [n, 4, 15] (SHADE_OUT)."""
    L = lib(fma)
    s1, s2, scr, fis = tables
    cap = (params.tile_w * params.tile_h * params.samples + 16) * (params.max_bounces + 2)
    pk, lane_u, lane_f = np.zeros((cap, 2), np.uint32), np.zeros((cap, 4, 4), np.uint32), np.zeros((cap, 4, 15), np.float32)
    out_u, out_f = np.zeros((cap, 4, 2), np.uint32), np.zeros((cap, 4, 15), np.float32)
    n = L.oracle_trace_shade(C.byref(world_desc), C.byref(params), _fp(s1), _fp(s2), _fp(scr), _fp(fis), tile_index, cap,
                             _up(pk), _up(lane_u), _fp(lane_f), _up(out_u), _fp(out_f))
    if n < 0 or n > cap:
        raise RuntimeError(f"oracle_trace_shade failed: {n}")
    return _shade_dict(pk[:n], lane_u[:n], lane_f[:n].copy(), out_u[:n], out_f[:n].copy())


def shade_packets(world_desc, params, tables, depth, obj, valid, sample, lane_f, fma=False, counts=False):
    """get_shading_info + Integrator::integrate on caller-built packets of one depth: obj [n], valid / sample [n, 4], lane_f [n, 4, 15] (SHADE_IN).
    -> (status [n, 4], aov [n, 4], out_f [n, 4, 15]); with counts=True a fourth item, the per-lane accounting of these packets as a dict over TALLY_KEYS."""
    L = lib(fma)
    s1, s2 = tables[0], tables[1]
    obj = np.ascontiguousarray(obj, np.uint32)
    n = len(obj)
    lane_u = np.zeros((n, 4, 4), np.uint32)
    lane_u[:, :, 0] = np.asarray(valid).reshape(n, 4) != 0
    lane_u[:, :, 1] = np.asarray(sample).reshape(n, 4)
    lane_f = np.ascontiguousarray(lane_f, np.float32).reshape(n, 4, 15)
    out_u, out_f = np.zeros((n, 4, 2), np.uint32), np.zeros((n, 4, 15), np.float32)
    tally = (C.c_uint64 * 13)()
    rc = L.oracle_shade_packets_counts(C.byref(world_desc), C.byref(params), _fp(s1), _fp(s2), depth, n, _up(obj), _up(lane_u), _fp(lane_f), _up(out_u), _fp(out_f), tally)
    if rc != 0:
        raise ValueError(f"oracle_shade_packets failed: {rc}")
    if counts:
        return out_u[:, :, 0].copy(), out_u[:, :, 1].copy(), out_f, {k: int(v) for k, v in zip(TALLY_KEYS, tally)}
    return out_u[:, :, 0].copy(), out_u[:, :, 1].copy(), out_f


def dump_scene(world_desc, params, path):
    """The scene blob oracle/shade_selftest.cpp reads: the bytes of rayn_world_desc, then of rayn_frame_params."""
    with open(path, "wb") as f:
        f.write(bytes(world_desc))
        f.write(bytes(params))


def sdf_dist(hitable, pts, fma=False, t0=None):
    """SDF::dist of one TracedSDF per point; t0 = lane 0's time of the calling packet, which only the MandelBox scale extension (scale_vel != 0) reads."""
    L = lib(fma)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), np.float32)
    if t0 is None:
        L.oracle_sdf_dist(C.byref(hitable), _fp(pts), _fp(out), C.c_uint64(len(pts)))
    else:
        L.oracle_sdf_dist_at(C.byref(hitable), C.c_float(t0), _fp(pts), _fp(out), C.c_uint64(len(pts)))
    return out


def closest_hit(world_desc, params, depth, org, dirs, fma=False):
    L = lib(fma)
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    t = np.zeros(len(org), np.float32)
    obj = np.zeros(len(org), np.uint32)
    L.oracle_closest_hit(C.byref(world_desc), C.byref(params), C.c_uint32(depth), _fp(org), _fp(dirs), _fp(t), _up(obj),
                         C.c_uint64(len(org)))
    return t, obj


def closest_hit_counts(world_desc, params, depth, org, dirs, fma=False):
    """closest_hit + per ray the SDF evaluations of the fold over every TracedSDF and the fold / orbit steps they ran: (t, obj, evals, steps)."""
    L = lib(fma)
    org = np.ascontiguousarray(org, np.float32).reshape(-1, 3)
    dirs = np.ascontiguousarray(dirs, np.float32).reshape(-1, 3)
    t = np.zeros(len(org), np.float32)
    obj, ev, it = (np.zeros(len(org), np.uint32) for _ in range(3))
    L.oracle_closest_hit_counts(C.byref(world_desc), C.byref(params), C.c_uint32(depth), _fp(org), _fp(dirs), _fp(t), _up(obj), _up(ev), _up(it),
                                C.c_uint64(len(org)))
    return t, obj, ev, it


def shadow_counts(world_desc, params, start, end, fma=False):
    """test_occluded + per segment what it costs as a parked shadow job: the evaluations (and their steps) of the TracedSDFs in index order, up to and
    including the first that occludes: (visibility, evals, steps)."""
    L = lib(fma)
    start = np.ascontiguousarray(start, np.float32).reshape(-1, 3)
    end = np.ascontiguousarray(end, np.float32).reshape(-1, 3)
    out = np.zeros(len(start), np.float32)
    ev, it = np.zeros(len(start), np.uint32), np.zeros(len(start), np.uint32)
    L.oracle_shadow_counts(C.byref(world_desc), C.byref(params), _fp(start), _fp(end), _fp(out), _up(ev), _up(it), C.c_uint64(len(start)))
    return out, ev, it


def render_jobs(world_desc, params, tables, fma=False):
    """render() on the calling thread with the job sink installed: (film, Counters, start [n, 3], end [n, 3]) - the segments of the frame's parked shadow jobs,
    in world coordinates, in the order they were parked."""
    L = lib(fma)
    L.oracle_set_job_sink(1)
    try:
        film, ctr = render(world_desc, params, tables, threads=1, fma=fma)
        n = int(L.oracle_take_job_sink(None, 0))
        seg = np.zeros((n // 6, 6), np.float32)
        L.oracle_take_job_sink(_fp(seg), n)
    finally:
        L.oracle_set_job_sink(0)
    return film, ctr, seg[:, 0:3].copy(), seg[:, 3:6].copy()


def sdf_steps(hitable, pts, fma=False):
    """Fold / orbit steps one evaluation of the TracedSDF runs at each point."""
    L = lib(fma)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    out = np.zeros(len(pts), np.uint32)
    L.oracle_sdf_steps(C.byref(hitable), _fp(pts), _up(out), C.c_uint64(len(pts)))
    return out


def test_occluded(world_desc, params, start, end, fma=False):
    L = lib(fma)
    start = np.ascontiguousarray(start, np.float32).reshape(-1, 3)
    end = np.ascontiguousarray(end, np.float32).reshape(-1, 3)
    out = np.zeros(len(start), np.float32)
    L.oracle_test_occluded(C.byref(world_desc), C.byref(params), _fp(start), _fp(end), _fp(out), C.c_uint64(len(start)))
    return out


def detmath(op, a, b=None, fma=False):
    L = lib(fma)
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(a if b is None else b, np.float32)
    out = np.zeros_like(a)
    L.oracle_detmath(C.c_uint32(op), _fp(a), _fp(b), _fp(out), C.c_uint64(a.size))
    return out


def detmath_core(op, a, b=None, fma=False):
    """The binary64 value the dm_* function of `op` (as detmath) hands to its final conversion to float; NaN where it answers without its core."""
    L = lib(fma)
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(a if b is None else b, np.float32)
    out = np.zeros(a.shape, np.float64)
    L.oracle_detmath_core(C.c_uint32(op), _fp(a), _fp(b), out.ctypes.data_as(C.POINTER(C.c_double)), C.c_uint64(a.size))
    return out


# floats per lane read / written by each op of oracle_probe_shading / rayn_hip_probe_shading (op table: include/rayn_hip.h)
SHADING_IN = (5, 2, 2, 3, 3, 2, 9, 3, 11, 5, 8, 1, 1, 8, 7)
SHADING_OUT = (6, 2, 3, 3, 9, 1, 3, 3, 7, 4, 2, 1, 1, 1, 1)


def probe_shading(world_desc, op, index, inp, aux=None, fma=False):
    """The oracle's own shading functions on n lanes of records (op table: include/rayn_hip.h): inp [n, SHADING_IN[op]] -> [n, SHADING_OUT[op]].
    aux = the 512-float inverse CDF of op 12."""
    L = lib(fma)
    inp = np.ascontiguousarray(inp, np.float32).reshape(-1, SHADING_IN[op])
    out = np.zeros((len(inp), SHADING_OUT[op]), np.float32)
    a = None if aux is None else np.ascontiguousarray(aux, np.float32)
    if a is not None:
        assert a.size == 512, a.size
    rc = L.oracle_probe_shading(C.byref(world_desc), C.c_uint32(op), C.c_uint32(index), _fp(inp), _fp(out),
                                None if a is None else _fp(a), C.c_uint64(len(inp)))
    if rc != 0:
        raise ValueError(f"oracle_probe_shading rejected op {op} index {index}")
    return out
