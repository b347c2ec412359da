"""Progressive rendering on the GPU (rayn_amd/csrc/progressive.hip, Film.render_progressive): the accumulate / compaction entries bit for
bit against the numpy restatement (tests/progressive_np.py; NaN payloads aside) on random and adversarial films, ragged tiles, sparse tile
lists and every switch; the whole loop against the restatement driven by the CPU oracle; resume; more than 16 384 spp; the multi-device
context; stream order; error codes and texts; the tile subset is cleared on every exit path."""
import ctypes as C

import numpy as np
import pytest

import device_io as IO
import progressive_cases as PC
import progressive_np as PN
from common import bits_equal
from progressive_cases import ADAPTIVE, BOUNCES, H, SAMPLES, TILE, W, oracle_epochs

pytestmark = pytest.mark.gpu
F32 = np.float32
GUARD = 16
SHAPES = [((1, 1), (1, 1)), ((7, 1), (4, 1)), ((17, 13), (8, 8)), ((33, 65), (16, 16)), ((300, 200), (64, 48)), ((300, 200), (16, 16))]


def _params(w, h, tile):
    import rayn_amd as R
    return R.frame_params(w, h, 1, 3, tile_size=tile)


def _dev(film, w, h, fill=None):
    """device film with GUARD guard floats behind every plane"""
    import torch
    out = {}
    for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
        out[key], view = IO.guarded(w * h * floats, torch.float32, 7.0, GUARD)  # the entries are handed the whole buffer
        if film is not None:
            view.copy_(torch.from_numpy(np.ascontiguousarray(film[key], F32).reshape(-1)))
        elif fill is not None:
            view.fill_(fill)
    return out


def _host(d, w, h):
    out = {}
    for key, floats in (("color", 3), ("alpha", 1), ("background", 3), ("normal", 3)):
        IO.assert_guards(d[key], w * h * floats, 7.0, f"the {key} plane")
        a = d[key][: w * h * floats].cpu().numpy()
        out[key] = a.reshape(-1, 3) if floats == 3 else a
    return out


def _assert_state(ctx, p, d_state, st, w, h, tile, what):
    from rayn_amd import progressive as P
    import torch
    torch.cuda.synchronize()
    raw = d_state.cpu().numpy()
    nbytes = P.state_bytes(w, h, tile)
    IO.assert_guards(d_state, nbytes, 0xA5, (what, "the state"))
    got = P.split_state(raw[:nbytes], w, h, tile)
    want = PC.restated_arrays(st)
    for k in P.STATE_FIELDS:
        if np.asarray(want[k]).dtype == np.float32:
            assert bits_equal(got[k], want[k]), (what, k)
        else:
            assert np.array_equal(got[k], want[k]), (what, k, got[k], want[k])
    assert got["active"].tolist() == st.active().tolist(), what
    active, totals = ctx.progressive_fetch_active(p, d_state)
    assert active.tolist() == st.active().tolist() and list(active) == sorted(active), what
    t = st.totals()
    assert totals["active_tiles"] == t["active_tiles"] and totals["outlier_pixels"] == t["outlier_pixels"], (what, totals, t)
    assert F32(totals["max_e"]).tobytes() == F32(t["max_e"]).tobytes(), (what, totals, t)
    rep = ctx.progressive_tile_report(p, d_state)
    assert np.array_equal(rep["epochs"], st.epochs) and np.array_equal(rep["retired"], st.retired) and np.array_equal(rep["outliers"], st.outliers)
    assert bits_equal(rep["max_e"], st.max_e), what


def _new_state(ctx, p, w, h, tile):
    import torch
    from rayn_amd import progressive as P
    d_state, _ = IO.guarded(P.state_bytes(w, h, tile), torch.uint8, 0xA5, 64)
    ctx.progressive_reset(p, d_state)
    return d_state


def test_accumulate_and_compaction_match_the_restatement(gpu_ctx):
    import rayn_amd as R
    switches = [dict(), dict(adaptive=False), dict(target_error=0.0, noise_floor=0.0, min_epochs=2, outlier_permille=0),
                dict(target_error=0.3, noise_floor=0.01, min_epochs=3, outlier_permille=500), dict(target_error=0.02, min_epochs=2, outlier_permille=1000),
                dict(target_error=1.0, noise_floor=1.0, min_epochs=2, outlier_permille=1)]
    for si, ((w, h), tile) in enumerate(SHAPES):
        p = _params(w, h, tile)
        n_tiles = len(PN.tile_rects(w, h, *tile))
        rng = np.random.default_rng(si)
        for sw_i, sw in enumerate(switches if w * h < 60000 else switches[:3]):
            prog = R.Progressive(**sw)
            kw = dict(target_error=prog.target_error, noise_floor=prog.noise_floor, min_epochs=prog.min_epochs, outlier_permille=prog.outlier_permille,
                      adaptive=prog.adaptive)
            st = PN.State(w, h, tile)
            d_state = _new_state(gpu_ctx, p, w, h, tile)
            _assert_state(gpu_ctx, p, d_state, st, w, h, tile, (w, h, tile, sw, "fresh"))
            d_mean = _dev(None, w, h, fill=5.0)
            st.mean = {k: np.full_like(v, 5.0) for k, v in st.mean.items()}  # pixels no epoch has reached keep what the caller's film held
            for epoch in range(1 + (si + sw_i) % 6):
                film = PC.film(w, h, 100 * si + 10 * sw_i + epoch, special=bool((epoch + sw_i) % 2))
                if epoch % 3 == 2:  # a low-noise epoch so that some tiles do retire
                    film = {k: (np.float32(0.5) + np.float32(1e-3) * v).astype(F32) for k, v in film.items()}
                tiles = None
                if epoch % 2 == 1 and n_tiles > 1:  # a sparse subset
                    tiles = np.sort(rng.choice(n_tiles, max(1, n_tiles // 3), replace=False)).astype(np.uint32)
                d_film = _dev(film, w, h)
                gpu_ctx.progressive_accumulate(p, prog, tiles, d_film, d_state, d_mean)
                PN.accumulate(st, film, tiles, **kw)
                what = (w, h, tile, sw, epoch, None if tiles is None else tiles.tolist())
                _assert_state(gpu_ctx, p, d_state, st, w, h, tile, what)
                got = _host(d_mean, w, h)
                after = _host(d_film, w, h)
                for k in PN.FILM_KEYS:
                    assert bits_equal(got[k], st.mean[k]), (what, "mean film", k)  # incl. the untouched pixels of unlisted tiles
                    assert np.array_equal(after[k].view(np.uint32), np.ascontiguousarray(film[k], F32).reshape(after[k].shape).view(np.uint32)), (what, "epoch film modified", k)


def _scene(name, w=W, h=H):
    import rayn_amd as R
    from rayn_amd import setup as S
    cam, world = S.SCENES[name]((w, h))
    return R, cam, world, R.PathTracingIntegrator(max_bounces=BOUNCES, volume_marches=S.VOLUME_MARCHES_PER_SAMPLE), R.BlackmanHarrisFilter(1.5)


def _film_host(film):
    return {k: film.channels[k].cpu().numpy() for k in PN.FILM_KEYS}


def _film_state(film):
    return film._progressive_arrays()[0]


def _assert_film_is_state(film, st, what):
    from rayn_amd import progressive as P
    got, want = _film_state(film), PC.restated_arrays(st)
    for k in P.STATE_FIELDS:
        assert bits_equal(got[k], want[k]) if np.asarray(want[k]).dtype == np.float32 else np.array_equal(got[k], want[k]), (what, k)
    host = _film_host(film)
    for k in PN.FILM_KEYS:
        assert bits_equal(host[k].reshape(st.mean[k].shape), st.mean[k]), (what, "mean film", k)


KINDS = lambda R: [R.ChannelKind.Color, R.ChannelKind.Alpha, R.ChannelKind.Background, R.ChannelKind.WorldNormal]


@pytest.mark.parametrize("name,fma", [("s1", False), ("s1", True), ("s2", False), ("s2", True)])
def test_the_loop_matches_the_oracle_driven_restatement(oracle, name, fma):
    R, cam, world, integ, filt = _scene(name)
    render_epoch, p = oracle_epochs(oracle, name, fma=fma)
    kw = dict(ADAPTIVE, max_epochs=12)
    st, hist = PN.run(render_epoch, W, H, TILE, 1, BOUNCES, p.volume_marches, **kw)
    assert len({len(h[2]) for h in hist}) > 2, "the scene does not adapt"
    film = R.Film(KINDS(R), (W, H))
    film.ctx.set_fma_policy(int(fma))
    seen = []
    rep = film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw),
                                  on_epoch=lambda r: seen.append((r["seed"], None if r["rendered_tiles"] is None else list(r["rendered_tiles"]), list(r["active_tiles"]))))
    assert rep["epochs"] == len(hist) == film.progressive_epoch
    for got, (s, subset, active) in zip(seen, hist):
        assert got == (s, None if subset is None else list(subset), list(active))
    assert np.array_equal(rep["tile_epochs"], st.epochs)
    _assert_film_is_state(film, st, (name, fma))
    assert rep["paths"] == int(st.epochs.sum()) * 256 * 4 * SAMPLES and rep["paths_non_adaptive"] == len(hist) * W * H * 4 * SAMPLES
    assert rep["paths"] < rep["paths_non_adaptive"]
    # the inspection images
    img = film.sample_count_image()
    assert img.shape == (H, W) and img.max() == 255 and len(np.unique(img)) > 2
    e = film.error_map()
    k = int(np.argmax(st.epochs))
    px = st.pixels_of(k)
    assert bits_equal(e.reshape(-1)[px], PN.e_p(st.mean_y[px], st.m2[px], int(st.epochs[k]), kw["noise_floor"]))
    # pixels / save_to work on the mean film unchanged
    assert film.pixels(R.ChannelKind.Color).shape == (H, W, 3)


def test_epoch_films_are_plain_renders_and_two_epochs_average(oracle):
    import torch
    R, cam, world, integ, filt = _scene("s1")
    kw = dict(ADAPTIVE, max_epochs=6)
    film = R.Film(KINDS(R), (W, H))
    epochs = []

    def grab(r):
        epochs.append((r["seed"], r["rendered_tiles"], {k: v.clone() for k, v in r["epoch_film"].items()}))
    film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw), on_epoch=grab)
    assert any(t is not None for _, t, _ in epochs)
    plain = R.Film(KINDS(R), (W, H))
    rects = PN.tile_rects(W, H, *TILE)
    for seed, tiles, got in epochs:
        # render_frame_into's film for that epoch's tables: frame = seed builds them; the time range stays the frame's
        plain.render_frame_into(world, cam, integ, filt, TILE, seed, (film._progressive["params"].time_start, film._progressive["params"].time_end), SAMPLES)
        for k in PN.FILM_KEYS:
            a = got[k].cpu().numpy().reshape(H, W, -1)
            b = plain.channels[k].cpu().numpy().reshape(H, W, -1)
            for t in (range(len(rects)) if tiles is None else tiles):
                x0, y0, x1, y1 = rects[t]
                assert bits_equal(a[y0:y1, x0:x1], b[y0:y1, x0:x1]), (seed, t, k)
    # min_epochs = max_epochs = 2: the mean film is (F0 + F1) / 2.0f
    two = R.Film(KINDS(R), (W, H))
    rep = two.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(min_epochs=2, max_epochs=2))
    assert rep["epochs"] == 2
    for k in PN.FILM_KEYS:
        f0, f1 = epochs[0][2][k].cpu().numpy(), epochs[1][2][k].cpu().numpy()
        assert epochs[1][1] is None
        assert bits_equal(two.channels[k].cpu().numpy(), (f0 + f1) / F32(2.0)), k
    # adaptive = False renders every tile in every epoch
    na = R.Film(KINDS(R), (W, H))
    rendered = []
    rep = na.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(kw, adaptive=False, max_epochs=4)),
                                on_epoch=lambda r: rendered.append(r["rendered_tiles"]))
    assert rendered == [None] * 4 and (rep["tile_epochs"] == 4).all() and rep["paths"] == rep["paths_non_adaptive"]
    assert all(s["tiles"] == len(rects) for s in rep["stats"])
    torch.cuda.synchronize()


def test_resume_equals_one_run(tmp_path, oracle):
    R, cam, world, integ, filt = _scene("s1")
    kw = dict(ADAPTIVE)
    one = R.Film(KINDS(R), (W, H))
    one.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(kw, max_epochs=6)))
    a = R.Film(KINDS(R), (W, H))
    rep = a.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(kw, max_epochs=3)))
    assert rep["epochs"] == 3
    path = str(tmp_path / "ck.npz")
    a.save_checkpoint(path)
    b = R.Film(KINDS(R), (W, H))
    seeds = []
    rep = b.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**dict(kw, max_epochs=6)), resume=path,
                               on_epoch=lambda r: seeds.append(r["seed"]))
    assert rep["epochs"] == 6 and seeds == [1 + e * 65536 for e in (3, 4, 5)] and len(rep["stats"]) == 3
    sa, sb = _film_state(one), _film_state(b)
    for k in sa:
        assert bits_equal(sa[k], sb[k]) if sa[k].dtype == np.float32 else np.array_equal(sa[k], sb[k]), k
    ha, hb = _film_host(one), _film_host(b)
    for k in PN.FILM_KEYS:
        assert bits_equal(ha[k], hb[k]), k
    # another world / frame / tile size
    R2, cam2, world2, _, _ = _scene("s2")
    c = R.Film(KINDS(R), (W, H))
    with pytest.raises(ValueError, match="another world"):
        c.render_progressive(world2, cam2, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw), resume=path)
    with pytest.raises(ValueError, match="another frame"):
        c.render_progressive(world, cam, integ, filt, TILE, 2, None, SAMPLES, R.Progressive(**kw), resume=path)
    with pytest.raises(ValueError, match="another tile_size"):
        c.render_progressive(world, cam, integ, filt, (8, 8), 1, None, SAMPLES, R.Progressive(**kw), resume=path)
    with pytest.raises(ValueError, match="no progressive render"):
        R.Film(KINDS(R), (W, H)).save_checkpoint(path)


def test_more_than_16384_spp(oracle):
    R, cam, world, integ, filt = _scene("s1", 16, 16)
    film = R.Film(KINDS(R), (16, 16))
    rep = film.render_progressive(world, cam, integ, filt, TILE, 1, None, 1024, R.Progressive(min_epochs=2, max_epochs=5, adaptive=False))
    assert rep["epochs"] == 5 and rep["paths"] == 5 * 4096 * 256 > 16384 * 256
    assert np.isfinite(film.channels["color"].cpu().numpy()).all()


def test_multi_device_context_gives_the_same_bits(oracle):
    R, cam, world, integ, filt = _scene("s1")
    kw = dict(ADAPTIVE, max_epochs=8)
    single = R.Film(KINDS(R), (W, H))
    single.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw))
    multi = R.Film(KINDS(R), (W, H))
    multi.ctx.close()
    multi.ctx = R.Context([0, 0])
    before = multi.ctx.table_broadcasts()
    rep = multi.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw))
    assert multi.ctx.table_broadcasts() - before >= rep["epochs"]  # every epoch's tables reached the peer
    sa, sb = _film_state(single), _film_state(multi)
    for k in sa:
        assert bits_equal(sa[k], sb[k]) if sa[k].dtype == np.float32 else np.array_equal(sa[k], sb[k]), k
    ha, hb = _film_host(single), _film_host(multi)
    for k in PN.FILM_KEYS:
        assert bits_equal(ha[k], hb[k]), k


def test_accumulate_is_stream_ordered(gpu_ctx, oracle):
    """The accumulate goes behind a render on a side stream with no host sync in between (render_device returns when the frame is
    complete, so copies queued behind it on the stream stand in for work still in flight)."""
    import torch
    import rayn_amd as R
    w, h, tile = 640, 360, (16, 16)
    p = _params(w, h, tile)
    film = PC.film(w, h, 3)
    st = PN.accumulate(PN.State(w, h, tile), film)
    src = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1)).cuda() for k, v in film.items()}
    from rayn_amd import progressive as P
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        d_state = torch.empty(P.state_bytes(w, h, tile), dtype=torch.uint8, device="cuda")
        gpu_ctx.progressive_reset(p, d_state, s.cuda_stream)
        dst = {k: torch.zeros_like(v) for k, v in src.items()}
        for k in dst:
            dst[k].copy_(src[k])  # queued on s before the accumulate: it must see the copied film, not zeros
        mean = {k: torch.zeros_like(v) for k, v in src.items()}
        gpu_ctx.progressive_accumulate(p, R.Progressive(), None, dst, d_state, mean, s.cuda_stream)
        host = {k: torch.empty(v.numel(), dtype=torch.float32, pin_memory=True) for k, v in mean.items()}
        for k in host:
            host[k].copy_(mean[k], non_blocking=True)
    s.synchronize()
    for k in PN.FILM_KEYS:
        assert bits_equal(host[k].numpy().reshape(st.mean[k].shape), st.mean[k]), k


def test_bad_arguments_return_invalid_arg_with_a_text(gpu_ctx):
    import torch
    from rayn_amd import _abi, _lib
    from rayn_amd import progressive as P
    L = _lib.lib()
    w, h, tile = 20, 12, (8, 8)
    p = _params(w, h, tile)
    need = P.state_bytes(w, h, tile)
    state = torch.zeros(need + 16, dtype=torch.uint8, device="cuda")
    film, mean = _dev(PC.film(w, h, 0), w, h), _dev(None, w, h)
    ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    n_tiles = len(PN.tile_rects(w, h, *tile))

    def call(p=p, pp=None, tiles=None, film=film, mean=mean, st=ptr(state), nbytes=need, **ppkw):
        pp = _abi.ProgressiveParams(0.05, 0.05, 4, 64, 50, 1) if pp is None else pp
        for k, v in ppkw.items():
            setattr(pp, k, v)
        arr = None if tiles is None else np.asarray(tiles, np.uint32)
        return L.rayn_hip_progressive_accumulate_device(gpu_ctx.h, C.byref(p), C.byref(pp), None if arr is None else arr.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                        0 if arr is None else len(arr), *[ptr(film.get(k)) for k in PN.FILM_KEYS], st, nbytes,
                                                        *[ptr(mean.get(k)) for k in PN.FILM_KEYS], s)

    def geom(**kw):
        q = _params(w, h, tile)
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    nan, inf = float("nan"), float("inf")
    small = "state smaller than rayn_progressive_state_bytes(width, height, tile_w, tile_h)"
    cases = [(dict(p=geom(width=0)), "zero-sized film"), (dict(p=geom(height=0)), "zero-sized film"), (dict(p=geom(tile_w=0)), "zero-sized tile"),
             (dict(p=geom(width=1 << 16, height=1 << 15)), "film larger than 2^31 pixels unsupported (32-bit pixel indices)"),
             (dict(tiles=[n_tiles]), "tile index beyond the film's tile count"), (dict(tiles=[0, 2, 1]), "tile list not strictly ascending"),
             (dict(tiles=[1, 1]), "tile list not strictly ascending"), (dict(tiles=[]), "empty tile list (pass NULL for every tile)"),
             (dict(st=None), "null buffer"), (dict(nbytes=need - 1), small), (dict(p=geom(tile_w=4)), small),
             (dict(st=C.c_void_p(state.data_ptr() + 4)), "state not 16-byte aligned"),
             (dict(min_epochs=1), "min_epochs must be >= 2"), (dict(max_epochs=3), "max_epochs must be >= min_epochs"),
             (dict(max_epochs=65537), "max_epochs must be <= 65536 (the epoch seeds of a frame)"),
             (dict(outlier_permille=1001), "outlier_permille must be <= 1000")]
    for v in (nan, inf, -inf, -0.5):
        cases += [(dict(target_error=v), "target_error must be finite and >= 0"), (dict(noise_floor=v), "noise_floor must be finite and >= 0")]
    for k in PN.FILM_KEYS:
        cases += [(dict(film=dict(film, **{k: None})), "null buffer"), (dict(mean=dict(mean, **{k: None})), "null buffer"),
                  (dict(mean=dict(mean, **{k: film[k]})), "the output film must not alias the epoch film")]
    for kwargs, text in cases:
        assert call(**kwargs) == -1, kwargs  # RAYN_ERR_INVALID_ARG
        assert gpu_ctx.last_error() == text, kwargs
    assert L.rayn_hip_progressive_reset_device(gpu_ctx.h, C.byref(p), ptr(state), need - 1, s) == -1 and gpu_ctx.last_error() == small
    assert L.rayn_hip_progressive_reset_device(None, C.byref(p), ptr(state), need, s) == -1
    assert L.rayn_hip_progressive_fetch_active(gpu_ctx.h, C.byref(p), None, need, None, 0, None, s) == -1 and gpu_ctx.last_error() == "null buffer"
    out = np.zeros(n_tiles, np.uint32)
    assert L.rayn_hip_progressive_fetch_active(gpu_ctx.h, C.byref(p), ptr(state), need, out.ctypes.data_as(C.POINTER(C.c_uint32)), n_tiles - 1, None, s) == -1
    assert gpu_ctx.last_error() == "out_tiles holds fewer entries than the film has tiles"
    assert L.rayn_hip_progressive_tile_report(gpu_ctx.h, C.byref(p), ptr(state), 0, None, None, None, None, s) == -1 and gpu_ctx.last_error() == small
    assert P.state_bytes(0, 4, tile) == 0 and P.state_bytes(4, 4, (0, 4)) == 0
    # good calls after the bad ones
    assert L.rayn_hip_progressive_reset_device(gpu_ctx.h, C.byref(p), ptr(state), need, s) == 0
    assert call() == 0 and call(tiles=[0, n_tiles - 1]) == 0 and call(target_error=0.0, noise_floor=-0.0, adaptive=0) == 0
    torch.cuda.synchronize()
    assert L.rayn_hip_progressive_fetch_active(gpu_ctx.h, C.byref(p), ptr(state), need, None, 0, None, s) == n_tiles


def test_the_tile_subset_is_cleared_on_every_exit_path(oracle):
    import torch
    R, cam, world, integ, filt = _scene("s1")
    kw = dict(ADAPTIVE, max_epochs=12)
    film = R.Film(KINDS(R), (W, H))
    n_tiles = len(PN.tile_rects(W, H, *TILE))

    def full_frame_renders(what):
        st = film.render_frame_into(world, cam, integ, filt, TILE, 1, None, SAMPLES)
        assert st["tiles"] == n_tiles, (what, st["tiles"])
    film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw))
    full_frame_renders("normal return")
    stopped = film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw),
                                      on_epoch=lambda r: not (r["rendered_tiles"] is not None))  # False once a subset has rendered
    assert stopped["rendered_tiles"] is not None and len(stopped["active_tiles"]) > 0
    full_frame_renders("on_epoch returned False")

    def boom(r):
        if r["rendered_tiles"] is not None:
            raise KeyError("from on_epoch")
    with pytest.raises(KeyError, match="from on_epoch"):
        film.render_progressive(world, cam, integ, filt, TILE, 1, None, SAMPLES, R.Progressive(**kw), on_epoch=boom)
    full_frame_renders("exception in on_epoch")
    torch.cuda.synchronize()
