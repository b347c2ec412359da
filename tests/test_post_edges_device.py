"""The progressive, a-trous and display kernels (rayn_amd/csrc/progressive.hip, denoise.hip, denoise_variance.hip, denoise_temporal.hip,
display.hip) at their decision edges on the GPU: every case of tests/post_edge_cases.py through every entry it applies to, every output
bit for bit against the numpy restatement (NaN payloads aside) - state planes, records, totals, active list and mean film; colour,
variance and history; float plane, 8-bit image, meter and bloom - with guard words behind every output and the inputs left alone, and
the hand-written outcomes against what the device wrote.  tests/test_post_edge_cases.py holds the cases to account on the CPU."""
import numpy as np
import pytest

import device_io as IO
import post_edge_cases as EC
import progressive_cases as PC
import progressive_np as PN
import temporal_np as T
from common import bits_equal

pytestmark = pytest.mark.gpu
f32 = np.float32
GUARD = 16
CASES = EC.all_cases()


def of(*families):
    cs = [c for c in CASES if c.family in families]
    return pytest.mark.parametrize("c", cs, ids=[c.name for c in cs])


def _params(w, h, tile=None):
    import rayn_amd as R
    return R.frame_params(w, h, 1, 3) if tile is None else R.frame_params(w, h, 1, 3, tile_size=tile)


def same(a, b):
    return bits_equal(np.asarray(a, f32).reshape(-1), np.asarray(b, f32).reshape(-1))


# ---- progressive ---------------------------------------------------------------------------------------------------------------------------
PLANES = (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3))


def _dev_film(film, n, fill=None):
    import torch
    out = {}
    for key, floats in PLANES:
        out[key], view = IO.guarded(n * floats, torch.float32, 7.0, GUARD)
        if film is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(film[key], f32).reshape(-1)))
        else:
            view.fill_(fill)
    return out


def _host_film(d, n):
    out = {}
    for key, floats in PLANES:
        IO.assert_guards(d[key], n * floats, 7.0, f"the {key} plane")
        a = d[key][: n * floats].cpu().numpy()
        out[key] = a.reshape(-1, 3) if floats == 3 else a
    return out


def _assert_state(ctx, p, d_state, st, c, what):
    """every word of the device state, the two host entries and the compaction against the restated state"""
    import torch
    from rayn_amd import progressive as P
    w, h, tile = c.w, c.h, c.tile
    torch.cuda.synchronize()
    raw = d_state.cpu().numpy()
    nbytes = P.state_bytes(w, h, tile)
    IO.assert_guards(d_state, nbytes, 0xA5, (what, "the state"))
    got, want = P.split_state(raw[:nbytes], w, h, tile), PC.restated_arrays(st)
    for k in P.STATE_FIELDS:
        if np.asarray(want[k]).dtype == np.float32:
            assert bits_equal(got[k], want[k]), (what, k)
        else:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["active"].tolist() == st.active().tolist(), what
    n, t = w * h, len(st.rects)
    totals = raw[48 * n + 16 * t: 48 * n + 16 * t + 16].view(np.uint32)
    tot = st.totals()
    assert (int(totals[0]), int(totals[2]) | int(totals[3]) << 32) == (tot["active_tiles"], tot["outlier_pixels"]), (what, totals)
    assert int(totals[1]) == EC.bits(tot["max_e"]), (what, totals)
    active, fetched = ctx.progressive_fetch_active(p, d_state)
    assert active.tolist() == st.active().tolist() and list(active) == sorted(active), what
    assert (fetched["active_tiles"], fetched["outlier_pixels"], EC.bits(fetched["max_e"])) == (tot["active_tiles"], tot["outlier_pixels"], EC.bits(tot["max_e"])), what
    rep = ctx.progressive_tile_report(p, d_state)
    assert np.array_equal(rep["epochs"], st.epochs) and np.array_equal(rep["retired"], st.retired) and np.array_equal(rep["outliers"], st.outliers), what
    assert bits_equal(rep["max_e"], st.max_e), what
    return rep, active, fetched


def check_tiles(c, rep, what):
    for k, (n, r, o, e) in c.expect.items():
        got = (int(rep["epochs"][k]), int(rep["retired"][k]), int(rep["outliers"][k]), EC.bits(rep["max_e"][k]))
        assert got == (n, r, o, EC.bits(e)), (c.name, what, "tile", k, got, (n, r, o, EC.bits(e)))


@of("progressive")
def test_progressive_cases(gpu_ctx, c):
    import torch
    import rayn_amd as R
    from rayn_amd import progressive as P
    w, h, tile, n = c.w, c.h, c.tile, c.w * c.h
    p = _params(w, h, tile)
    prog = R.Progressive(max_epochs=65536, **c.params)
    d_state, view = IO.guarded(P.state_bytes(w, h, tile), torch.uint8, 0xA5, 64)
    if c.init is None:
        st = PN.State(w, h, tile)
        gpu_ctx.progressive_reset(p, d_state)
    else:
        st = c.init()
        view.copy_(torch.from_numpy(P.join_state(PC.restated_arrays(st), w, h, tile)))
    _assert_state(gpu_ctx, p, d_state, st, c, (c.name, "before"))
    d_mean = _dev_film(None, n, fill=5.0)
    st.mean = {k: np.full_like(v, 5.0) for k, v in st.mean.items()}  # pixels no epoch reaches keep what the caller's film held
    for i, film in enumerate(c.films):
        d_film = _dev_film(film, n)
        gpu_ctx.progressive_accumulate(p, prog, c.tiles, d_film, d_state, d_mean)
        PN.accumulate(st, film, c.tiles, **c.params)
        rep, active, fetched = _assert_state(gpu_ctx, p, d_state, st, c, (c.name, i))
        got, after = _host_film(d_mean, n), _host_film(d_film, n)
        for k in PN.FILM_KEYS:
            assert bits_equal(got[k], st.mean[k]), (c.name, i, "mean film", k)
            assert IO.same_bits(after[k], np.ascontiguousarray(film[k], f32).reshape(after[k].shape)), (c.name, i, "epoch film modified", k)
    # the hand-written outcome against what the device reports
    check_tiles(c, rep, "tile report")
    if hasattr(c, "active"):
        assert active.tolist() == c.active
        assert (fetched["active_tiles"], EC.bits(fetched["max_e"]), fetched["outlier_pixels"]) == (c.totals[0], EC.bits(c.totals[1]), c.totals[2])
    for q, v in getattr(c, "mean_color", {}).items():
        assert (got["color"][q] == f32(v)).all(), (c.name, q, got["color"][q])


@of("progressive_wide")
def test_the_wide_tile(gpu_ctx, c):
    """More than 4 294 967 pixels in one tile: outliers * 1000 needs 64 bits.  The planes are filled on the device and the outcome is the
    hand-written one; the state's planes are compared with the single value every pixel holds."""
    import torch
    import rayn_amd as R
    from rayn_amd import progressive as P
    w, h, tile, n = c.w, c.h, c.tile, c.w * c.h
    p = _params(w, h, tile)
    prog = R.Progressive(max_epochs=64, **c.params)
    nbytes = P.state_bytes(w, h, tile)
    d_state, _ = IO.guarded(nbytes, torch.uint8, 0xA5, 64)
    gpu_ctx.progressive_reset(p, d_state)
    d_film, d_mean = _dev_film(None, n, fill=0.0), _dev_film(None, n, fill=5.0)
    for gray in c.grays:
        d_film["color"][: 3 * n].fill_(gray)
        gpu_ctx.progressive_accumulate(p, prog, None, d_film, d_state, d_mean)
    torch.cuda.synchronize()
    IO.assert_guards(d_state, nbytes, 0xA5, "the state")
    rep = gpu_ctx.progressive_tile_report(p, d_state)
    check_tiles(c, rep, "tile report")
    active, totals = gpu_ctx.progressive_fetch_active(p, d_state)
    assert active.tolist() == [0] and (totals["active_tiles"], totals["outlier_pixels"], EC.bits(totals["max_e"])) == (1, n, 0x3F800000)
    planes = d_state[: 48 * n].view(torch.float32).reshape(3, n, 4)
    # sums (1, 1, 1, 0), (0, 0, 0), (0, 0, 0); mean_y = 0.5 and m2 = 0.5 in every pixel; the mean film is (0.5, 0.5, 0.5), 0, 0, 0
    for plane, want in zip(planes, ((1.0, 1.0, 1.0, 0.0), (0.0, 0.0, 0.0, 0.5), (0.0, 0.0, 0.0, 0.5))):
        assert bool(torch.all(plane == torch.tensor(want, device="cuda"))), want
    for (key, floats), want in zip(PLANES, (0.5, 0.0, 0.0, 0.0)):
        IO.assert_guards(d_mean[key], n * floats, 7.0, key)
        IO.assert_guards(d_film[key], n * floats, 7.0, key)
        assert bool(torch.all(d_mean[key][: n * floats] == want)), key
    assert bool(torch.all(d_film["color"][: 3 * n] == c.grays[-1]))


# ---- the a-trous family --------------------------------------------------------------------------------------------------------------------

def _guides(c):
    film = {"color": c.color, "normal": c.normal, "alpha": c.alpha}
    return IO.upload_film(film, ("color",) + (("normal",) if c.sigmas[1] else ()) + (("alpha",) if c.sigmas[2] else ()))


def check_weights(c, col):
    if hasattr(c, "keeps"):
        w0 = f32(9.0 / 64.0)
        assert same(col[c.keeps], (w0 * np.asarray(c.color, f32).reshape(-1, 3)[c.keeps]) / w0)
        assert (col[c.positive_zero] == 0).all() and not np.signbit(col[c.positive_zero]).any()


@of("denoise")
def test_denoise_cases(gpu_ctx, oracle, c):
    import torch
    from rayn_amd import Denoise
    n = c.w * c.h
    d = _guides(c)
    keep = IO.snapshot(d)
    full, out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
    gpu_ctx.denoise(c.w, c.h, d, out, Denoise(c.iterations, *c.sigmas))
    torch.cuda.synchronize()
    IO.assert_guards(full, 3 * n, 7.0, "colour")
    IO.assert_unchanged(d, keep, "an input")
    got = out.cpu().numpy().reshape(n, 3)
    IO.assert_bits_equal(got, EC.run_denoise(c), (c.name, "colour"))
    if hasattr(c, "centre"):
        assert same(got[c.centre], [c.centre_colour] * 3)
    check_weights(c, got)


@of("vdenoise")
def test_variance_denoiser_cases(gpu_ctx, oracle, c):
    import torch
    from rayn_amd import VarianceDenoise
    from rayn_amd import progressive as P
    n = c.w * c.h
    d = _guides(c)
    raw = P.join_state(c.state, c.w, c.h, c.tile)
    d_state, view = IO.guarded(raw.size, torch.uint8, 0xA5, 64)
    view.copy_(torch.from_numpy(raw))
    ins = dict(d, state=d_state)
    keep = IO.snapshot(ins)
    want_c, want_v, v0 = EC.run_vdenoise(c)
    for variance in (False, True):  # the variance output is optional; the pass with it comes last and is the one looked at below
        full_out, out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
        full_var, var = IO.guarded(n, torch.float32, 7.0, GUARD)
        gpu_ctx.denoise_variance(_params(c.w, c.h, c.tile), d, d_state, out, VarianceDenoise(c.iterations, *c.sigmas), var if variance else None)
        torch.cuda.synchronize()
        IO.assert_guards(full_out, 3 * n, 7.0, "colour")
        IO.assert_guards(full_var, n if variance else 0, 7.0, "variance")
        IO.assert_unchanged(ins, keep, "an input")
        got_c, got_v = out.cpu().numpy().reshape(n, 3), var.cpu().numpy()
        IO.assert_bits_equal(got_c, want_c, (c.name, "colour", variance))
        if variance:
            IO.assert_bits_equal(got_v, want_v, (c.name, "variance"))
            assert np.array_equal(np.isnan(got_v), np.isnan(want_v))
    # the hand-written outcome against what the device wrote
    if hasattr(c, "v0"):
        known = c.v0 != -1
        guided = ~np.isnan(c.v0[known])
        assert (np.isnan(got_v[known]) == ~guided).all(), (c.name, "guided")
        assert same(got_c[known][~guided], np.asarray(c.color, f32).reshape(-1, 3)[known][~guided])
    if hasattr(c, "centre"):
        assert same(got_c[c.centre], [c.centre_colour] * 3) and same(got_v[c.centre], c.centre_variance)
    check_weights(c, got_c)
    for q, v in getattr(c, "variance", {}).items():
        assert same(got_v[q], v), (c.name, q, got_v[q], v)
    for q, v in getattr(c, "colour", {}).items():
        assert (got_c[q] == f32(v)).all(), (c.name, q, got_c[q])
    for q in getattr(c, "not_guided", []):
        assert np.isnan(got_v[q])


@of("tvdenoise")
def test_temporal_variance_cases(gpu_ctx, oracle, c):
    """Both entries: rayn_hip_denoise_temporal_variance_device (strength 0) and the feedback one at the case's strength, or at 0.5"""
    import torch
    from rayn_amd import VarianceDenoise
    n = c.w * c.h
    d = _guides(c)
    g = {"object": IO.upload(c.obj.view(np.int32), np.int32)}
    hist_bytes = np.ascontiguousarray(T.join_history(*c.hist))
    d_mom = IO.upload_bytes(c.mom)
    ins = dict(d, object=g["object"], mom=d_mom)
    keep = IO.snapshot(ins)
    hb = len(hist_bytes)
    first = None
    for beta in (0.0, c.beta or 0.5):
        want_c, want_v, _, _, want_A = EC.run_tvdenoise(c, beta=beta)
        arena = torch.full((hb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
        d_hist = arena[GUARD: GUARD + hb]
        d_hist.copy_(torch.from_numpy(hist_bytes))
        full_out, out = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
        full_var, var = IO.guarded(n, torch.float32, 7.0, GUARD)
        gpu_ctx.denoise_temporal_variance(c.w, c.h, d, g, d_hist, d_mom, out, VarianceDenoise(c.iterations, *c.sigmas), var, feedback=beta)
        torch.cuda.synchronize()
        assert bool(torch.all(arena[:GUARD] == 0xA5)), "a kernel wrote in front of the history"
        IO.assert_guards(arena, GUARD + hb, 0xA5, "history")
        IO.assert_guards(full_out, 3 * n, 7.0, "colour")
        IO.assert_guards(full_var, n, 7.0, "variance")
        IO.assert_unchanged(ins, keep, "an input")
        got_c, got_v = out.cpu().numpy().reshape(n, 3), var.cpu().numpy()
        IO.assert_bits_equal(got_c, want_c, (c.name, beta, "colour"))
        IO.assert_bits_equal(got_v, want_v, (c.name, beta, "variance"))
        assert np.array_equal(np.isnan(got_v), np.isnan(want_v))
        A, B, N, O = T.split_history(d_hist.cpu().numpy(), n)
        assert IO.same_bits(A, want_A), (c.name, beta, "plane A of the history")  # strict: the untouched words keep their bits
        assert IO.same_bits(A[:, 3], c.hist[0][:, 3]) and IO.same_bits(B, c.hist[1]) and IO.same_bits(N, c.hist[2]) and np.array_equal(O, c.hist[3])
        if beta == 0.0:
            assert IO.same_bits(A, c.hist[0])
            first = (got_c, got_v)
        else:
            assert IO.same_bits(got_c, first[0]) and IO.same_bits(got_v, first[1]), (c.name, "the feedback entry's outputs")
    # the hand-written outcome against what the device wrote
    if hasattr(c, "lone"):
        assert EC.bits(got_v[c.lone]) == EC.bits(c.lone_variance)
    guided = ~np.isnan(c.v0[c.v0 != -1])
    assert (np.isnan(got_v[c.v0 != -1]) == ~guided).all()
    if c.beta:
        changed = (A.view(np.uint32) != c.hist[0].view(np.uint32)).any(axis=1)
        assert not changed[c.keeps].any() and changed[c.takes].all() and same(A[c.takes, :3], got_c[c.takes])


# ---- display -------------------------------------------------------------------------------------------------------------------------------

def _display(ctx, c):
    """Both entries through Context.display, every output followed by guard words: the float plane, the image, {m, e}, the bloom plane
    (None without bloom) and the state afterwards"""
    import torch
    from rayn_amd.film import display_scratch_bytes, save_to_bpp
    film, w, h, display = c.film, c.w, c.h, c.display
    d = IO.upload_film(film)
    keep = IO.snapshot(d)
    n = w * h
    mask = 1 | (2 if film.get("alpha") is not None else 0) | (4 if film.get("background") is not None else 0)
    bpp = save_to_bpp(0, mask, c.transparent)
    need = display_scratch_bytes(w, h, display.levels)
    states, outs = [], {}
    before = np.array([f32(c.state[0]).view(np.int32), c.state[1]], np.int32)
    for key, dtype, count, fill in (("d", torch.float32, 3 * n, 7.0), ("image", torch.uint8, n * bpp, 0x5A)):
        full_out, out = IO.guarded(count, dtype, fill, GUARD)
        full_meter, meter = IO.guarded(2, torch.float32, 7.0, GUARD)
        full_bloom, bloom = IO.guarded(3 * n, torch.float32, 7.0, GUARD)
        full_scratch, _ = IO.guarded(need, torch.uint8, 0xAB, 64)
        full_st, st = IO.guarded(2, torch.int32, 0x55, GUARD)
        st.copy_(torch.from_numpy(before))
        ctx.display(display, mask, c.transparent, w, h, d, full_out, full_st, full_scratch, c.adapt, full_meter, full_bloom)
        torch.cuda.synchronize()
        for whole, size, word, name in ((full_out, count, fill, key), (full_meter, 2, 7.0, "meter"), (full_bloom, 3 * n if display.levels else 0, 7.0, "bloom"),
                                        (full_scratch, need, 0xAB, "scratch"), (full_st, 2, 0x55, "state")):
            IO.assert_guards(whole, size, word, (c.name, name))
        IO.assert_unchanged(d, keep, "an input")
        out, meter, bloom, st = (t.cpu().numpy() for t in (out, meter, bloom, st))
        if not display.auto:
            assert np.array_equal(st, before)
        outs[key] = out
        states.append((st, meter, bloom))
    for a, b in zip(states[0], states[1]):  # both entries meter, adapt and bloom alike
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    st, meter, bloom = states[0]
    return {"d": outs["d"].reshape(n, 3), "image": outs["image"].reshape(h, w, bpp), "meter": meter,
            "bloom": bloom.reshape(n, 3) if display.levels else None, "state": (st[:1].view(f32)[0], int(st[1]))}


@of("display")
def test_display_cases(gpu_ctx, oracle, c):
    got, want = _display(gpu_ctx, c), EC.run_display(c)
    IO.assert_bits_equal(got["d"], want["d"], (c.name, "float plane"))
    assert np.array_equal(got["image"], want["image"]), (c.name, "image", int((got["image"] != want["image"]).sum()))
    IO.assert_bits_equal(got["meter"], [want["m"], want["e"]], (c.name, "m, e"))
    if c.display.levels:
        IO.assert_bits_equal(got["bloom"], want["bloom"], (c.name, "bloom"))
    assert got["state"][1] == (want["state"][1] if c.display.auto else c.state[1]), c.name
    if c.display.auto:
        IO.assert_bits_equal([got["state"][0]], [want["state"][0]], (c.name, "state"))
    # the hand-written outcome against what the device wrote
    e = c.expect
    if "e" in e:
        assert got["meter"][1] == f32(e["e"])
    if "state" in e:
        assert same(got["state"][0], e["state"][0]) and got["state"][1] == e["state"][1]
    if "m" in e and e["m"] is not None:
        m = oracle.detmath(6, np.array([2.0], f32))[0] if isinstance(e["m"], str) else e["m"]
        assert same(got["state"][0], m) and same(got["meter"][0], m) and got["state"][1] == 1, (c.name, got["state"], m)
    for q, rgb in e.get("d", {}).items():
        assert same(got["d"][q], rgb) and (np.signbit(got["d"][q]) == np.signbit(np.asarray(rgb, f32))).all(), (c.name, q, got["d"][q], rgb)
    for q, v in e.get("image", {}).items():
        assert (got["image"][c.h - 1 - q // c.w, q % c.w, :3] == v).all(), (c.name, q, v)
    if e.get("bloom_zero"):
        assert (got["bloom"] == 0).all() and not np.signbit(got["bloom"]).any()
    if "bloom_value" in e:
        assert got["bloom"][e["bloom_value"][0]] == f32(e["bloom_value"][1]), (c.name, got["bloom"][e["bloom_value"][0]])
    if "bloom_inf" in e:
        assert np.isposinf(got["bloom"][e["bloom_inf"]])
    if "bloom_all" in e:
        assert (got["bloom"] == f32(e["bloom_all"])).all(), (c.name, got["bloom"])
