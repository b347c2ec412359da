"""The oracle's packet entry (oracle_py.shade_packets) and recorder (oracle_py.trace_shade) against the renderer they wrap, and every case of
tests/shade_cases.py against the condition it names - judged from the oracle's outputs and the case's inputs, without a GPU.  The device tests
(tests/test_shade_device.py) compare the product kernels with exactly these outputs."""
import numpy as np
import pytest

import shade_cases as SC
from common import bits_equal
from oracle.oracle_py import SH_BACKGROUND, SH_COLOR, SH_INVALID, SH_SPAWNED, SHADE_IN, SHADE_OUT

POLICIES = [False, True]


def _same_bits(a, b):
    return bool((np.ascontiguousarray(a, np.float32).view(np.uint32) == np.ascontiguousarray(b, np.float32).view(np.uint32)).all())


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("name", SC.RECORDED_SCENES)
def test_shade_packets_returns_what_the_renderer_recorded(oracle, name, fma):
    """every depth of the recorded tile: the same inputs through shade_packets give the recorded outputs, bit for bit (NaN payloads included: same code, same machine)"""
    sc = SC.scene(name)
    scr = sc["tabs"][2]
    assert SC.depths(name) and SC.depths(name)[0] == 0
    for d in SC.depths(name):
        case = SC.recorded(name, d, fma)
        st, aov, of = SC.expect(case, fma)
        rst, raov, rof = SC.recorded_outputs(name, d, fma)
        assert (st == rst).all() and (aov == raov).all(), (name, d)
        assert _same_bits(of, rof), (name, d)
        v = case["valid"]
        assert (st[~v] == SH_INVALID).all() and (st[v] != SH_INVALID).all()
        assert v[:, 0].all(), "lane 0 of a bin packet is always a real hit"
        assert _same_bits(case["lane_f"][v][:, SHADE_IN["scramble"]], scr[case["pix"][v]]), "a lane's scramble is its pixel's"
        assert (case["sample"][~v] == 0).all() and _same_bits(case["lane_f"][~v][:, SHADE_IN["scramble"]], np.zeros(int((~v).sum()), np.float32))


@pytest.mark.parametrize("fma", POLICIES)
@pytest.mark.parametrize("name", ["ship", "two_sdfs", "anim_spheres"])
def test_recorded_samples_are_the_film(oracle, name, fma):
    """summed per pixel in record order and divided by the sample count, the recorded samples are the tile of oracle.render: the recorder is tied to the film"""
    sc, tr = SC.scene(name), SC.trace(name, fma)
    film, _ = oracle.render(sc["wd"], sc["p"], sc["tabs"], threads=1, tile_subset=[SC.TILE_INDEX], fma=fma)
    x0, y0 = tr["origin"]
    acc = {k: np.zeros((SC.TILE, SC.TILE, 3), np.float32) for k in ("color", "background", "normal")}
    alpha = np.zeros((SC.TILE, SC.TILE), np.float32)
    one = np.float32(1.0)
    for k in range(len(tr["obj"])):              # record order = emission order: Alpha + WorldNormal of a packet first, then its Color / Background samples
        for i in range(4):
            if tr["aov"][k, i]:
                alpha[tr["tcy"][k, i], tr["tcx"][k, i]] += one
                acc["normal"][tr["tcy"][k, i], tr["tcx"][k, i]] += tr["out_f"][k, i, SHADE_OUT["normal"]]
        for i in range(4):
            if tr["status"][k, i] in (SH_COLOR, SH_BACKGROUND):
                plane = acc["color" if tr["status"][k, i] == SH_COLOR else "background"]
                plane[tr["tcy"][k, i], tr["tcx"][k, i]] += tr["out_f"][k, i, SHADE_OUT["radiance"]]
    n = np.float32(4 * sc["p"].samples)
    sl = (slice(y0, y0 + SC.TILE), slice(x0, x0 + SC.TILE))
    for k in acc:
        assert bits_equal(acc[k] / n, film[k][sl]), (name, k)
    assert bits_equal(alpha / n, film["alpha"][sl])
    assert len(np.unique(film["alpha"][sl])) >= 2, "the recorded tile shows the fractal and the sky"


def test_recorded_scenes_are_what_they_are_named_for(oracle):
    assert SC.scene("ship")["ns"] == 12 and SC.scene("ship")["n_lights"] == 5 and SC.scene("s1")["ns"] == 4
    assert SC.scene("lights8")["n_lights"] == 8 and SC.scene("lights8")["p"].volume_marches == 2
    assert SC.scene("lights3_vm4")["n_lights"] == 3 and SC.scene("lights3_vm4")["ns"] == 20
    assert SC.scene("no_lights_vol")["n_lights"] == 0 and SC.scene("no_lights_vol")["wd"].has_scattering
    assert SC.scene("ship_b0")["p"].max_bounces == 0 and SC.depths("ship_b0") == [0]
    assert SC.depths("spheres_only") == [0]
    marching = tuple(n for n in SC.RECORDED_SCENES if SC.scene(n)["n_lights"] > 0
                     and any(h.kind == 1 for h in list(SC.scene(n)["wd"].hitables)[:SC.scene(n)["wd"].n_hitables]))  # a TracedSDF and a light
    assert marching == SC.SDF_SCENES and len(marching) == 8
    tr = SC.trace("anim_spheres")                # the lanes of a packet have different times, and the moving ball is hit
    t = tr["lane_f"][:, :, SHADE_IN["time"]]
    assert ((t[:, 1:] != t[:, :1]) & (tr["valid"][:, 1:] != 0)).any() and (tr["obj"] == len(SC.scene("anim_spheres")["receives"]) - 1).any()
    for name in SC.RECORDED_SCENES:              # every recorded scene has spawned, terminated and padding lanes somewhere
        st = SC.trace(name)["status"]
        if name not in ("spheres_only", "ship_b0"):
            assert (st == SH_SPAWNED).any()
        assert (st == SH_INVALID).any() and ((st == SH_COLOR) | (st == SH_BACKGROUND)).any(), name


def _io(name, fma):
    case = SC.build(name)
    return case, SC.expect(case, fma)


@pytest.mark.parametrize("fma", POLICIES)
def test_roulette_cases(oracle, fma):
    recv = None
    for d in (2, 3, SC.BOUNCES):
        case, (st, _, _) = _io(f"roulette_d{d}", fma)
        recv = SC._receiving(case)[:, None] & case["valid"]
        assert set(np.unique(case["cmax"]).tolist()) == {0.0, 0.5, 1.0, 4.0}
        term, spawned = (st == SH_COLOR) & recv, (st == SH_SPAWNED) & recv
        if d == 2:
            assert spawned.any() and not term.any()
        elif d == 3:
            assert spawned.any() and term.any()
            assert spawned[case["cmax"] == 4.0].any(), "a bright path survives the roulette"
            assert term[case["cmax"] == 0.0].any(), "a black path loses it with probability 1"
        else:
            assert term.any() and not spawned.any()


@pytest.mark.parametrize("fma", POLICIES)
def test_zero_throughput_cases(oracle, fma):
    """zero_thr lanes leave the radiance bit-equal to radiance + the Le term alone (on a light-receiving hit: the radiance itself), and still spawn"""
    for name in ("zero_thr", "zero_thr_all", "zero_thr_bound_at", "zero_thr_bound_above"):  # (ordinary lights: every NEE term is finite)
        case, (st, _, of) = _io(name, fma)
        m = case["marked"]
        assert m.any() and (name != "zero_thr" or (case["valid"] & ~m).any())
        assert _same_bits(case["lane_f"][m][:, SHADE_IN["throughput"]], np.zeros((int(m.sum()), 3), np.float32))
        assert _same_bits(of[m][:, SHADE_OUT["radiance"]], case["lane_f"][m][:, SHADE_IN["radiance"]]), name  # Le * 0 = 0, and every NEE term is an exact zero
        recv = SC._receiving(case)[:, None] & m
        assert (st[recv] == SH_SPAWNED).all() and (name not in ("zero_thr", "zero_thr_all") or recv.any())
        assert _same_bits(of[recv][:, SHADE_OUT["throughput"]], np.zeros((int(recv.sum()), 3), np.float32))
    a, b = SC.scene("bound_at")["wd"], SC.scene("bound_above")["wd"]
    two60 = np.float32(2.0) ** 60
    assert all(L.emission.x == two60 and L.emission.y == two60 and L.emission.z == two60 for L in list(a.lights)[:a.n_lights])
    assert b.lights[1].emission.x == np.nextafter(two60, np.float32(np.inf)) and not a.has_extinction and not b.has_extinction
    # the pdf side: |equi-angular pdf x light pdf| of every light lies inside the binade above 2^-60 in one case and inside the one below in the other, whatever
    # the sample - by the oracle's own light functions (ops 10 and 9 of the shading probe)
    sc = SC.scene("far_open")
    wd = sc["wd"]
    assert not sc["receives"][1] and not wd.has_extinction and all(h.kind == 1 or h.radius < 1.0 for h in list(wd.hitables)[:wd.n_hitables]), "no sky sphere"
    for name, lo in (("zero_thr_pdf_above", -60), ("zero_thr_pdf_below", -61)):
        case, (st, _, of) = _io(name, fma)
        v = case["valid"]
        assert (st[v] == SH_COLOR).all() and (case["obj"] == 1).all()
        assert _same_bits(of[v][:, SHADE_OUT["radiance"]], case["lane_f"][v][:, SHADE_IN["radiance"]]), name
        t = case["lane_f"][v][:, SHADE_IN["t"]]
        org, d = case["lane_f"][v][:, SHADE_IN["origin"]], case["lane_f"][v][:, SHADE_IN["dir"]]
        for light in range(sc["n_lights"]):
            for u in (0.03, 0.5, 0.97):
                vol = oracle.probe_shading(wd, 10, light, np.concatenate([np.full((len(t), 1), u, np.float32), org, d, t[:, None]], 1), fma=fma)
                lpdf = oracle.probe_shading(wd, 9, light, np.concatenate([np.full((len(t), 2), u, np.float32), org + d * vol[:, :1]], 1), fma=fma)[:, 3]
                pdf = np.abs(vol[:, 1].astype(np.float64) * lpdf)
                assert (pdf > 2.0 ** lo * 1.15).all() and (pdf < 2.0 ** (lo + 1) / 1.15).all(), (name, light, u, np.log2(pdf.min()), np.log2(pdf.max()))
    # huge_lights (the construction of tests/test_gpu_parity.py): samples outside the x bound reach the radiance as inf * 0 = NaN on some lanes, not on all
    case, (st, _, of) = _io("zero_thr_huge_lights", fma)
    rad = of[case["marked"]][:, SHADE_OUT["radiance"]]
    assert np.isnan(rad).any() and np.isfinite(rad).all(1).any()


@pytest.mark.parametrize("fma", POLICIES)
def test_special_value_cases(oracle, fma):
    for name, field, pred in (("nan_thr", "throughput", np.isnan), ("inf_thr", "throughput", np.isinf), ("inf_rad", "radiance", np.isinf),
                              ("denormal_thr", "throughput", lambda x: (x != 0) & (np.abs(x) < np.finfo(np.float32).tiny))):
        case, (st, _, of) = _io(name, fma)
        m = case["marked"]
        assert all(m[:, i].any() for i in range(4)), (name, "the lanes 0..3 in turn")
        assert (pred(case["lane_f"][m][:, SHADE_IN[field]]).sum(1) == 1).all(), name
        sp = m & (st == SH_SPAWNED)
        assert sp.any() and (m & (st == SH_COLOR)).any(), name
        if name == "nan_thr":  # the NaN product is refused: the spawned ray keeps the old throughput, NaN and all
            assert bits_equal(of[sp][:, SHADE_OUT["throughput"]], case["lane_f"][sp][:, SHADE_IN["throughput"]])
        if name == "inf_rad":
            assert np.isinf(of[m][:, SHADE_OUT["radiance"]]).any(1).all()


@pytest.mark.parametrize("fma", POLICIES)
def test_geometry_cases(oracle, fma):
    case, (st, _, of) = _io("neg_t", fma)
    m = case["marked"]
    assert m.sum() >= 8 and (case["lane_f"][m][:, SHADE_IN["t"]] < 0).all() and (case["lane_f"][case["valid"] & ~m][:, SHADE_IN["t"]] > 0).any()
    assert SC.scene("bulbv")["wd"].hitables[1].sdf_kind == 2, "the Mandelbulb"
    assert (st[m] == SH_SPAWNED).any()
    # in_light: a shading point at a light's centre, on its surface, inside it - at least one non-finite radiance, and not all of them
    case, (st, _, of) = _io("in_light", fma)
    rad = of[case["marked"]][:, SHADE_OUT["radiance"]]
    assert (~np.isfinite(rad)).any() and np.isfinite(rad).all(1).any()
    # grazing: dot(normal, wi) is exactly +0 at the top point and exactly -0 at the bottom point, recomputed here from the case's inputs, the oracle's own
    # WorldNormal sample and its own light sample (op 9 of the shading probe), in the order of the oracle's dot, unfused and fused.  The light on the tangent
    # plane adds exact zeros and the other one lies behind the surface, so the radiance of every lane is the one it came with.
    case, (st, aov, of) = _io("grazing", fma)
    m = case["marked"]
    wd = SC.scene("ball")["wd"]
    f32, f64 = np.float32, np.float64
    assert {int(x) for x in case["valid"].sum(1)} == {1, 2, 3, 4} and aov[m].all()
    for bottom, light, want_sign in ((False, 0, False), (True, 1, True)):
        sel = m & (case["bottom"] == bottom)[:, None]
        assert sel.sum() >= 8
        point = case["lane_f"][sel][:, SHADE_IN["origin"]]       # t = 0
        n = of[sel][:, SHADE_OUT["normal"]]
        assert _same_bits(n, np.broadcast_to(np.array([0.0, -1.0 if bottom else 1.0, 0.0], f32), n.shape))
        for u in (0.0, 0.31, 0.97):
            end = oracle.probe_shading(wd, 9, light, np.concatenate([np.full((len(point), 2), u, f32), point], 1), fma=fma)[:, :3]
            wi = end - point
            wi = wi / np.sqrt((wi.astype(f64) ** 2).sum(1)).astype(f32)[:, None]
            assert (wi[:, 0] < 0).all() and _same_bits(wi[:, 1], np.zeros(len(wi), f32)) and ((wi[:, 2] < 0) == bottom).all()
            unfused = n[:, 0] * wi[:, 0] + (n[:, 1] * wi[:, 1] + n[:, 2] * wi[:, 2])
            fused = (n[:, 0].astype(f64) * wi[:, 0] + (n[:, 1].astype(f64) * wi[:, 1] + (n[:, 2] * wi[:, 2]).astype(f64)).astype(f32)).astype(f32)
            for d in (unfused, fused):
                assert (d == 0).all() and (np.signbit(d) == want_sign).all(), (bottom, u, d)
    assert _same_bits(of[m][:, SHADE_OUT["radiance"]], case["lane_f"][m][:, SHADE_IN["radiance"]])
    assert (st[m] == SH_SPAWNED).all()
    assert bits_equal(of[m][:, SHADE_OUT["origin"]], case["lane_f"][m][:, SHADE_IN["origin"]])
    # far: exp(-rho_t t) = 0 on the marked packets: a spawned ray's throughput is exactly 0 there, and not on the denormal ones
    case, (st, _, of) = _io("far", fma)
    m, v = case["marked"], case["valid"]
    sp, sp_den = m & (st == SH_SPAWNED), v & ~m & (st == SH_SPAWNED)
    assert sp.any() and sp_den.any()
    assert _same_bits(of[sp][:, SHADE_OUT["throughput"]], np.zeros((int(sp.sum()), 3), np.float32))
    thr_den = of[sp_den][:, SHADE_OUT["throughput"]]
    assert ((thr_den != 0) & (np.abs(thr_den) < np.finfo(np.float32).tiny)).any(), "a denormal throughput survives"


def test_bins_cases(oracle):
    """waves (16 packets) with mixed receives_light, packets of 1, 2 and 3 valid lanes, and a wave without any receiving packet"""
    for name in ("bins", "bins_dark_wave"):
        case = SC.build(name)
        assert SC.scene(case["scene"])["ns"] == 4
        recv = SC._receiving(case)
        waves = [recv[k:k + 16] for k in range(0, len(recv), 16)]
        assert any(w.any() and not w.all() for w in waves), name
        assert {1, 2, 3, 4} <= {int(x) for x in case["valid"].sum(1)}
        assert case["valid"][:, 0].all()
        if name == "bins_dark_wave":
            assert not waves[0].any() and len(waves[0]) == 16
        else:
            assert recv[0] == False and recv[15] == True and (~recv[16:32]).any() and recv[16:32].any()
        st, _, _ = SC.expect(case, False)
        assert (st == SH_SPAWNED).any() and (st == SH_BACKGROUND).any() and (st == SH_INVALID).any()


def test_second_trip_exceeds_both_trip_thresholds():
    """on stand-ins for the library's limits (the device test takes the real ones from rayn_hip_probe_shade_limits)"""
    blocks, ids, ns = 2048, 256 * 64, SC.scene("ship_vm4")["ns"]
    assert ns == 20
    n = SC.second_trip_slots(blocks, ids, ns)
    assert n % 64 == 0 and ns * n > blocks * ids and ns * (n - 64) <= blocks * ids and n > blocks * 256
    assert len(SC.second_trip_base()["obj"]) > 64


@pytest.mark.parametrize("fma", POLICIES)
def test_every_group_keeps_its_statuses_under_both_policies(oracle, fma):
    for name in SC.MUTATED:
        case, (st, _, _) = _io(name, fma)
        v = case["valid"]
        assert (st[v] != SH_INVALID).all() and (st[~v] == SH_INVALID).all(), name
        if not name.startswith(("zero_thr_bound", "zero_thr_pdf", "grazing", f"roulette_d{SC.BOUNCES}")):  # (sky hits only / every lane spawns / every lane ends)
            assert (st == SH_SPAWNED).any() and ((st == SH_COLOR) | (st == SH_BACKGROUND)).any(), name


def test_pool_encoding_round_trips():
    for case in (SC.recorded("ship", 1), SC.build("bins"), SC.fit(SC.recorded("ship", 0), 64), SC.fit(SC.recorded("ship", 2), 320)):
        scr = SC.scene(case["scene"])["tabs"][2]
        pool = SC.to_pool(case)
        back = SC.from_pool(pool, scr)
        n, v = len(case["obj"]), case["valid"]
        assert pool["n_slots"] % 64 == 0 and len(pool["ref"]) == pool["n_slots"] and 4 * n <= pool["n_slots"]
        assert (back["valid"][:n] == v).all() and not back["valid"][n:].any()
        assert (back["obj"][:n][v] == np.broadcast_to(case["obj"][:, None], v.shape)[v]).all()
        assert (back["sample"][:n][v] == case["sample"][v]).all() and (back["pix"][:n][v] == case["pix"][v]).all()
        assert _same_bits(back["lane_f"][:n][v], case["lane_f"][v])
        named = pool["ref"][pool["ref"] != SC.INVALID]
        assert len(np.unique(named)) == len(named) == int(v.sum()) and len(pool["free"]) == SC.EXTRA_RECORDS
        assert not np.array_equal(np.sort(named), named), "the pool order is unrelated to the slot order"
    tiled = SC.to_pool(SC.recorded("ship", 2), tile_to=1024)
    assert (tiled["ref"] != SC.INVALID).sum() == len(tiled["P"]) and tiled["packet"].max() == len(SC.recorded("ship", 2)["obj"]) - 1
