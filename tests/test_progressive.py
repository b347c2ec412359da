"""Progressive rendering on the CPU (no GPU needed): the epoch seed, the numpy restatement (tests/progressive_np.py) on hand-made films,
the oracle-driven adaptive loop, the calibration of the error estimate, the `Progressive` parameters and the checkpoint file."""
import dataclasses

import numpy as np
import pytest

import progressive_cases as PC
import progressive_np as PN
from common import bits_equal
from progressive_cases import ADAPTIVE, BOUNCES, H, TILE, W, oracle_epochs

F32 = np.float32

# ---- seed --------------------------------------------------------------------------------------------------------------------------

def test_epoch_zero_is_the_plain_frame():
    import rayn_amd as R
    for frame in (0, 1, 77):
        assert R.progressive_seed(frame, 0, 3, 2) == frame == PN.seed(frame, 0, 3, 2)
        a = R.film.build_rd_tables(8, 3, 2, R.progressive_seed(frame, 0, 3, 2))
        b = R.film.build_rd_tables(8, 3, 2, frame)
        assert all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(a, b))
    for frame, epoch in ((1, 1), (5, 9), (65535, 65535)):
        assert R.progressive_seed(frame, epoch, 3, 2) == frame + epoch * 65536 == PN.seed(frame, epoch, 3, 2)


def _sets(tables, spp):
    s1, s2 = tables
    return [r.tobytes() for r in s1.reshape(-1, spp)] + [r.tobytes() for r in s2.reshape(-1, 2 * spp)]


@pytest.mark.parametrize("bounces,vm", [(3, 2), (120, 2)])
def test_epochs_share_no_sample_set(bounces, vm):
    import rayn_amd as R
    spp, frame = 4, 1
    per_epoch = [set(_sets(R.film.build_rd_tables(spp, bounces, vm, R.progressive_seed(frame, e, bounces, vm)), spp)) for e in range(4)]
    for a in range(4):
        for b in range(a + 1, 4):
            assert not per_epoch[a] & per_epoch[b], (a, b)
    # frame and frame + 1 DO share sets (all but one 1-D set, shifted by one): the reason for the stride
    s1a, _ = R.film.build_rd_tables(spp, bounces, vm, frame)
    s1b, _ = R.film.build_rd_tables(spp, bounces, vm, frame + 1)
    rows_a, rows_b = s1a.reshape(-1, spp), s1b.reshape(-1, spp)
    assert np.array_equal(rows_a[1:], rows_b[:-1])


def test_seed_overflow_and_too_many_sets_are_errors():
    import rayn_amd as R
    assert R.progressive_seed(65535, 65535, 3, 2) == 2 ** 32 - 1
    assert R.progressive_seed(1, 3, 120, 58) == 1 + 3 * 65536  # 3 + 121 * (15 + 9 * 58) = 64980 sets
    for args in ((65536, 65535, 3, 2), (0, 65536, 3, 2), (2 ** 32 - 1, 1, 3, 2), (1, 1, 120, 59), (1, 0, 120, 59)):
        with pytest.raises(ValueError):
            R.progressive_seed(*args)
        with pytest.raises(ValueError):
            PN.seed(*args)
    with pytest.raises(ValueError):
        R.progressive_seed(2 ** 32, 0, 3, 2)


# ---- the restatement on hand-made films -----------------------------------------------------------------------------------------------

def test_one_epochs_mean_film_is_the_films_bits():
    w, h = 19, 11
    film = PC.film(w, h, 0, special=True)
    film["color"][0] = -0.0
    st = PN.accumulate(PN.State(w, h, (8, 8)), film)
    covered = np.concatenate([st.pixels_of(k) for k in range(len(st.rects))])
    assert len(covered) < w * h  # 19 = 2 * 8 + 3: the reference's tile list leaves the last 3 columns uncovered
    for key in PN.FILM_KEYS:
        assert bits_equal(st.mean[key][covered], film[key][covered]), key
        assert bits_equal(st.sum[key][covered], film[key][covered]), key
    assert np.signbit(st.mean["color"][0]).all()  # -0 stays -0
    assert not st.outliers.any() and not st.max_e.any() and not st.retired.any() and (st.epochs == 1).all()


def test_counts_and_max_do_not_depend_on_pixel_order():
    rng = np.random.default_rng(1)
    e = rng.gamma(1.0, 0.1, 500).astype(F32)
    e[::7] = np.nan
    e[::11] = 0.0
    e[3] = np.inf
    want = PN.tile_report(e, 0.1)
    for i in range(5):
        got = PN.tile_report(rng.permutation(e), 0.1)
        assert got[0] == want[0] and F32(got[1]).tobytes() == F32(want[1]).tobytes()
    assert want[1] == np.inf and want[0] == int(np.nansum(e > F32(0.1)))
    assert PN.tile_report(np.array([np.nan, np.nan], F32), 0.1) == (0, 0)


def test_nan_inf_and_negative_zero_behave_as_defined():
    w, h = 4, 4
    st = PN.State(w, h, (4, 4))
    base = {"color": np.full((16, 3), 0.5, F32), "alpha": np.ones(16, F32), "background": np.zeros((16, 3), F32), "normal": np.zeros((16, 3), F32)}
    films = [dict(base, color=base["color"].copy()) for _ in range(3)]
    films[1]["color"][0, 0] = np.nan   # pixel 0: NaN from epoch 1 on
    films[1]["color"][1, 1] = np.inf   # pixel 1: inf
    films[0]["color"][2] = -0.0        # pixel 2: -0 once, then 0.5
    for i, f in enumerate(films):
        PN.accumulate(st, f, target_error=0.01, noise_floor=0.0, min_epochs=2, outlier_permille=0)
        if i == 0:
            assert st.retired[0] == 0  # never before min_epochs
    assert np.isnan(st.mean_y[0]) and np.isnan(st.m2[0]) and np.isnan(st.mean["color"][0, 0])
    e = PN.e_p(st.mean_y, st.m2, 3, 0.0)
    assert np.isnan(e[0]) and np.isnan(e[1])  # inf - inf in the Welford step
    # the NaN pixels hold nothing open: only pixel 2 (a real outlier) counts
    assert st.outliers[0] == 1 and e[2] > 0.01 and st.max_e[0] == e[2]
    assert st.retired[0] == 0
    # a constant pixel with a zero floor: se = 0, e = 0 / 0.5 = 0; with mean 0 too, 0 / 0 = NaN and no outlier
    st0 = PN.State(1, 1, (1, 1))
    zero = {"color": np.zeros((1, 3), F32), "alpha": np.zeros(1, F32), "background": np.zeros((1, 3), F32), "normal": np.zeros((1, 3), F32)}
    for _ in range(2):
        PN.accumulate(st0, zero, target_error=0.0, noise_floor=0.0, min_epochs=2, outlier_permille=0)
    assert st0.outliers[0] == 0 and st0.max_e[0] == 0 and st0.retired[0] == 1


def test_retirement_at_the_permille_boundary():
    # 16x16 tile = 256 pixels, 50 permille: 12 outliers -> 12000 <= 12800 retires, 13 -> 13000 > 12800 does not
    assert PN.retires(4, 12, 256, 4, 50) and not PN.retires(4, 13, 256, 4, 50)
    assert not PN.retires(3, 0, 256, 4, 50)  # min_epochs
    assert PN.retires(4, 256, 256, 4, 1000) and not PN.retires(4, 1, 256, 4, 0) and PN.retires(4, 0, 256, 4, 0)
    assert PN.retires(2, 1, 1000, 2, 1) and not PN.retires(2, 2, 1000, 2, 1)  # exactly one per thousand
    # through accumulate: k noisy pixels in a 16x16 tile
    for k, want in ((12, 1), (13, 0)):
        st = PN.State(16, 16, (16, 16))
        for epoch in range(4):
            f = {"color": np.full((256, 3), 0.5, F32), "alpha": np.ones(256, F32), "background": np.zeros((256, 3), F32), "normal": np.zeros((256, 3), F32)}
            f["color"][:k] = epoch % 2
            PN.accumulate(st, f, target_error=0.05, noise_floor=0.05, min_epochs=4, outlier_permille=50)
        assert st.outliers[0] == k and st.retired[0] == want
    # retired stays retired; adaptive=False retires nothing
    st = PN.State(16, 16, (16, 16))
    f = {"color": np.full((256, 3), 0.5, F32), "alpha": np.ones(256, F32), "background": np.zeros((256, 3), F32), "normal": np.zeros((256, 3), F32)}
    for _ in range(3):
        PN.accumulate(st, f, min_epochs=2, adaptive=False)
    assert st.retired[0] == 0
    PN.accumulate(st, f, min_epochs=2)
    noisy = dict(f, color=np.random.default_rng(0).uniform(0, 9, (256, 3)).astype(F32))
    PN.accumulate(st, noisy, min_epochs=2)
    assert st.retired[0] == 1 and st.outliers[0] > 100


def test_unlisted_tiles_are_left_alone():
    w, h = 40, 24
    st = PN.State(w, h, (16, 16))
    PN.accumulate(st, PC.film(w, h, 2))
    before = {k: v.copy() for k, v in st.sum.items()}
    mean_before = {k: v.copy() for k, v in st.mean.items()}
    PN.accumulate(st, PC.film(w, h, 3), tiles=[1, 2])
    other = np.concatenate([st.pixels_of(k) for k in (0, 3, 4, 5)])  # 40x24 in 16x16 tiles: 3 x 2 tiles
    for key in PN.FILM_KEYS:
        assert bits_equal(st.sum[key][other], before[key][other]) and bits_equal(st.mean[key][other], mean_before[key][other])
    assert st.epochs.tolist() == [1, 2, 2, 1, 1, 1]


# ---- the oracle-driven loop ---------------------------------------------------------------------------------------------------------

def test_the_oracle_driven_loop_adapts(oracle):
    render_epoch, p = oracle_epochs(oracle, "s1")
    rendered = []

    def counting(seed, subset):
        rendered.append(None if subset is None else list(subset))
        return render_epoch(seed, subset)
    st, hist = PN.run(counting, W, H, TILE, 1, BOUNCES, p.volume_marches, **ADAPTIVE)
    m = ADAPTIVE["min_epochs"]
    print("tile epochs", st.epochs.tolist(), "active per epoch", [len(h[2]) for h in hist])
    assert (st.epochs == m).any(), "no tile retired at min_epochs"
    assert len(hist) >= m + 2 and len(hist[m + 1][2]) >= 1, "no tile was still active two epochs later"
    assert len(hist) < ADAPTIVE["max_epochs"] and st.retired.all(), "the run did not end before max_epochs"
    # a retired tile is never rendered again, the seeds are those of the epochs, the active lists ascend
    for e, (s, subset, active) in enumerate(hist):
        assert s == 1 + e * 65536 and list(active) == sorted(active)
        assert rendered[e] == (None if subset is None else list(subset))
        assert all(st.epochs[k] > e for k in (range(len(st.rects)) if subset is None else subset))
    assert sum(len(st.rects) if r is None else len(r) for r in rendered) == int(st.epochs.sum())


def test_non_adaptive_renders_every_tile_every_epoch(oracle):
    render_epoch, p = oracle_epochs(oracle, "s1")
    st, hist = PN.run(render_epoch, W, H, TILE, 1, BOUNCES, p.volume_marches, **dict(ADAPTIVE, max_epochs=4, adaptive=False))
    assert len(hist) == 4 and all(h[1] is None for h in hist) and (st.epochs == 4).all() and not st.retired.any()
    # with two epochs the mean film is (F0 + F1) / 2 in f32
    f0, f1 = PN.flat(render_epoch(1, None)), PN.flat(render_epoch(1 + 65536, None))
    st2, _ = PN.run(render_epoch, W, H, TILE, 1, BOUNCES, p.volume_marches, min_epochs=2, max_epochs=2)
    for key in PN.FILM_KEYS:
        assert bits_equal(st2.mean[key], (f0[key] + f1[key]) / F32(2.0)), key


# ---- calibration of the error estimate -------------------------------------------------------------------------------------------------

# predicted / observed variance of mean_y measured on the oracle at 48x32, 4 spp per epoch, 8 epochs
MEASURED_RATIOS = {"s1": 1.152, "s2": 1.085, "s3": 0.993}


def test_the_error_estimate_is_calibrated(oracle):
    """Non-adaptive, E = 8 epochs: the predicted variance of a pixel's mean luminance (mean over the pixels of se^2 = m2 / (E (E - 1)))
    against the observed one (half the mean squared difference of mean_y between two runs of E epochs: epochs 0..E-1 and E..2E-1 of the
    frame, i.e. frames that differ by E strides, so no epoch of one run shares a table with one of the other).  1 for independent epochs.
    The band is [min / 1.5, max * 1.5] of the three measured ratios (the margin covers scene-to-scene spread, nothing else); measured
    ratios outside [0.5, 2] would be a finding about the seeds."""
    E = 8
    assert all(0.5 <= r <= 2.0 for r in MEASURED_RATIOS.values())
    lo, hi = min(MEASURED_RATIOS.values()) / 1.5, max(MEASURED_RATIOS.values()) * 1.5
    for name in MEASURED_RATIOS:
        render_epoch, p = oracle_epochs(oracle, name)
        runs = [PN.run(render_epoch, W, H, TILE, frame, BOUNCES, p.volume_marches, min_epochs=2, max_epochs=E, adaptive=False)[0]
                for frame in (1, 1 + E * PN.STRIDE)]
        predicted = np.mean([np.mean(s.m2.astype(np.float64) / (E * (E - 1))) for s in runs])
        observed = 0.5 * np.mean((runs[0].mean_y.astype(np.float64) - runs[1].mean_y) ** 2)
        ratio = predicted / observed
        print(f"{name}: predicted {predicted:.4e} observed {observed:.4e} ratio {ratio:.3f}")
        assert lo <= ratio <= hi, (name, ratio, lo, hi)


# ---- parameters and the checkpoint file --------------------------------------------------------------------------------------------------

def test_progressive_parameters_are_validated():
    import rayn_amd as R
    R.Progressive()
    R.Progressive(0.0, 2, 2, 0, 0.0, False)
    R.Progressive(max_epochs=65536, outlier_permille=1000)
    for kw in (dict(min_epochs=1), dict(min_epochs=5, max_epochs=4), dict(max_epochs=65537), dict(outlier_permille=1001), dict(outlier_permille=-1),
               dict(target_error=-0.1), dict(target_error=float("nan")), dict(target_error=float("inf")), dict(noise_floor=-1.0),
               dict(noise_floor=float("nan")), dict(noise_floor=1e39), dict(min_epochs=2.0), dict(min_epochs=True), dict(adaptive=1),
               dict(target_error="x")):
        with pytest.raises(ValueError):
            R.Progressive(**kw)
    with pytest.raises(dataclasses.FrozenInstanceError):
        R.Progressive().min_epochs = 3


def test_checkpoint_round_trip_and_key_mismatches(tmp_path):
    import rayn_amd as R
    from rayn_amd import progressive as P
    from rayn_amd import setup as S
    w, h, tile = 40, 24, (16, 16)
    st = PN.State(w, h, tile)
    for i in range(3):
        PN.accumulate(st, PC.film(w, h, i, special=True), tiles=None if i < 2 else [0, 3], min_epochs=2, target_error=10.0, outlier_permille=1000)
    arrays = PC.restated_arrays(st)
    cam, world = S.setup_s1((w, h))
    args = dict(resolution=(w, h), tile_size=tile, samples=2, max_bounces=3, volume_marches=2, frame=7, time_range=(0.25, 0.5),
                filter=R.BlackmanHarrisFilter(1.5), world_bytes=world.to_desc(cam), progressive=R.Progressive(), fma_policy=0)
    key = P.checkpoint_key(**args)
    path = str(tmp_path / "ck")  # no .npz suffix: the name is kept as given
    P.write_checkpoint(path, key, arrays, 3)
    key2, arrays2, epochs = P.read_checkpoint(path)
    assert epochs == 3
    P.check_key(key2, key)
    for k in P.STATE_FIELDS:
        assert arrays2[k].dtype == np.asarray(arrays[k]).dtype and arrays2[k].tobytes() == np.asarray(arrays[k]).tobytes(), k
    # the device state blob: split(join(x)) == x, the active list is that of the records, and the layout has the documented size
    raw = P.join_state(arrays, w, h, tile)
    assert raw.size == P.state_bytes(w, h, tile) == 48 * w * h + 16 * 6 + 16 + 8 * 6  # 3 x 2 tiles
    back = P.split_state(raw, w, h, tile)
    for k in P.STATE_FIELDS:
        assert back[k].tobytes() == np.asarray(arrays[k]).tobytes(), k
    assert back["active"].tolist() == st.active().tolist()
    mean = P.mean_film(arrays, w, h, tile)
    covered = np.concatenate([st.pixels_of(k) for k in range(6)])
    for k in PN.FILM_KEYS:
        assert bits_equal(mean[k][covered], st.mean[k][covered]), k
    # the inspection images
    e = P.error_map(arrays, w, h, tile, 0.05).reshape(-1)
    for k in range(6):
        assert bits_equal(e[st.pixels_of(k)], PN.e_p(st.mean_y[st.pixels_of(k)], st.m2[st.pixels_of(k)], int(st.epochs[k]), 0.05))
    img = P.sample_count_image(st.epochs, w, h, tile)
    assert img.shape == (h, w) and img.dtype == np.uint8 and img[h - 1, 0] == 255 and img[h - 1 - 16, 0] == 170 and img[0, w - 1] == 170
    # every field of the key is reported by name
    cam2, world2 = S.setup_s2((w, h))
    other = dict(resolution=(w, h + 1), tile_size=(8, 16), samples=3, max_bounces=4, volume_marches=3, frame=8, time_range=(0.25, 0.75),
                 filter=R.BoxFilter(1.5), world_bytes=world2.to_desc(cam2), fma_policy=1)
    for name, value in other.items():
        with pytest.raises(ValueError, match="another " + {"world_bytes": "world"}.get(name, name)):
            P.check_key(key2, P.checkpoint_key(**dict(args, **{name: value})))
    for name, value in dict(target_error=0.06, noise_floor=0.01, min_epochs=5, outlier_permille=51, adaptive=False).items():
        with pytest.raises(ValueError, match="another " + name):
            P.check_key(key2, P.checkpoint_key(**dict(args, progressive=dataclasses.replace(R.Progressive(), **{name: value}))))
    P.check_key(key2, P.checkpoint_key(**dict(args, progressive=R.Progressive(max_epochs=9))))  # max_epochs does not affect retirement
    assert set(P.KEY_FIELDS) == set(key)
    bad = tmp_path / "bad.npz"
    np.savez(str(bad), x=np.zeros(3))
    with pytest.raises(ValueError, match="not a progressive checkpoint"):
        P.read_checkpoint(str(bad))
