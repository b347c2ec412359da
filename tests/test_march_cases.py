"""tests/march_cases.py checked without a GPU: the sizing rule against a simulation of the chunk hand-out, the layout of the corner classes, the threaded
oracle helpers against the plain calls, and what the oracle itself makes of the generated inputs (so that a steady-state comparison on the GPU compares
something: both outcomes, several objects, the NaN classes ending as the kernel comments say)."""
import numpy as np
import pytest

import march_cases as M

CHUNK, ENDGAME = 256, 256 * 32 * 64  # stand-ins: the GPU tests take the real ones from rayn_hip_probe_march_limits


def _first_bases(n, chunk, waves):
    """Brute force: every wave of the grid takes its first chunk (one atomicAdd(head, chunk) each, in any order); the bases that lie inside the queue."""
    head, bases = 0, []
    for _ in range(waves):
        base, head = head, head + chunk
        if base < n:
            bases.append(base)
    return bases


@pytest.mark.parametrize("blocks,k,extra", [(2048, 1, 0), (2048, 3, 0), (64, 1, 3), (64, 2, 3), (64, 4, 3), (1, 1, 0), (7, 3, 2)])
def test_steady_n_puts_every_first_fetch_in_steady_state(blocks, k, extra):
    n = M.steady_n(CHUNK, ENDGAME, blocks, k, extra)
    waves = 4 * blocks
    assert (n + CHUNK - 1) // CHUNK > blocks  # the grid is capped by `blocks`, not by the queue (stride_grid)
    bases = _first_bases(n, CHUNK, waves * (1 + extra))  # 1 + extra rounds of the whole grid
    assert len(bases) == waves * (1 + extra)
    assert all(n - base >= k * ENDGAME for base in bases)  # the kernels' endgame test is n - base < k * ENDGAME
    assert n % 64 == 37 and n % CHUNK != 0                 # padding entries and a last partial chunk
    # one entry short of the threshold: every chunk is an endgame chunk
    assert not any(k * ENDGAME - 1 - base >= k * ENDGAME for base in _first_bases(k * ENDGAME - 1, CHUNK, waves))
    # and the queue does reach its endgame after the steady part: the chunks of the last k * ENDGAME entries
    assert (n - (n // CHUNK) * CHUNK) < k * ENDGAME


def test_endgame_only_below_the_threshold():
    n = ENDGAME - 1
    assert all(n - base < ENDGAME for base in _first_bases(n, CHUNK, 4 * 2048))
    assert 40000 < ENDGAME and 30000 < ENDGAME  # the sizes of the older probe tests: endgame only


@pytest.mark.parametrize("gen,classify,names", [(M.segments, M.seg_class, M.SEG_CLASSES), (M.rays, M.ray_class, M.RAY_CLASSES)])
def test_every_corner_class_in_every_window(gen, classify, names):
    n = 5 * M.WINDOW + 229
    c = classify(np.arange(n))
    assert abs((c >= 0).mean() - 1.0 / 8.0) < 0.001
    for lo in range(0, n - M.WINDOW + 1, 61):  # unaligned windows too
        assert set(np.unique(c[lo:lo + M.WINDOW])) == set(range(-1, len(names))), lo
    assert np.array_equal(c[M.WINDOW:2 * M.WINDOW], c[:M.WINDOW])  # i % WINDOW names the class
    x, y = gen(n, 5)
    assert x.shape == y.shape == (n, 3) and x.dtype == y.dtype == np.float32
    assert not x.flags.writeable and not y.flags.writeable
    assert gen(n, 5)[0] is x  # cached
    # the classes are what their names say, and the ordinary entries are finite
    ordinary = c < 0
    assert np.isfinite(x[ordinary]).all() and np.isfinite(y[ordinary]).all()
    k = lambda name: c == names.index(name)
    if gen is M.segments:
        assert np.isnan(x[k("nan_start"), 0]).all() and np.isinf(x[k("inf_start"), 1]).all() and np.isnan(y[k("nan_end"), 2]).all()
        assert np.array_equal(x[k("zero_length")], y[k("zero_length")])
        assert (np.abs(x[k("far_start")]).max(axis=1) > 2.0).mean() > 0.9 and np.abs(y[k("end_inside")]).max() <= 0.1
        assert np.signbit(x[k("neg_zero_start")]).all() and (x[k("neg_zero_start")] == 0).all() and np.signbit(y[k("neg_zero_end")]).all()
        d = np.abs(x[k("near_coincident")] - y[k("near_coincident")]).max()
        assert 0 < d < 2e-5
    else:
        assert np.isnan(x[k("nan_origin"), 0]).all() and np.isinf(x[k("inf_origin"), 2]).all() and np.isnan(y[k("nan_dir"), 1]).all()
        assert (y[k("zero_dir")] == 0).all() and np.signbit(x[k("neg_zero_origin")]).all() and (x[k("neg_zero_origin")] == 0).all()
        assert (np.abs(x[k("far_origin")]).max(axis=1) > 3.0).mean() > 0.9
        assert np.abs(np.linalg.norm(y[ordinary].astype(np.float64), axis=1) - 1.0).max() < 1e-6


@pytest.mark.parametrize("name", ["s1", "bulb"])
def test_threaded_oracle_equals_the_plain_calls(oracle, name):
    n = 20000
    a, b = M.segments(n, 7)
    wd, p = M.probe_world(name, sdf_only=True)
    assert np.array_equal(M.oracle_test_occluded_mt(oracle, wd, p, a, b), oracle.test_occluded(wd, p, a, b))
    assert np.array_equal(M.oracle_test_occluded_mt(oracle, wd, p, a, b, threads=3), oracle.test_occluded(wd, p, a, b))
    org, d = M.rays(n, 8)
    wd, p = M.probe_world(name)
    for depth in (0, 2):
        t, obj = M.oracle_closest_hit_mt(oracle, wd, p, depth, org, d)
        rt, robj = oracle.closest_hit(wd, p, depth, org, d)
        assert np.array_equal(obj, robj) and np.array_equal(t.view(np.uint32), rt.view(np.uint32))
    assert 1 <= M.cpus() <= 16


@pytest.mark.parametrize("name", ["s1", "s0", "bulb"])
def test_oracle_outcomes_on_the_generated_inputs(oracle, name):
    """From the reference alone, at a reduced n with the generators of the GPU tests: both shadow outcomes occur, the rays hit several objects, and the NaN
    classes end as the kernel comments promise - a NaN first distance, and NaN later distances (which are never 'occluded' / never a hit and run out the
    march budget), leave a segment visible and a ray without an SDF hit (and a NaN origin or direction misses every analytic sphere too: no object, t_max)."""
    n = 200000 + 37
    wd, p, a, b, ref = M.occluded_case(oracle, name, {}, 31, n)
    assert M.occluded_case(oracle, name, {}, 31, n)[4] is ref  # the oracle ran once
    assert set(np.unique(ref)) == {0.0, 1.0}
    occluded = 1.0 - float(ref.mean())
    print(name, "occluded share", occluded)
    assert 0.02 < occluded < 0.98
    c = M.seg_class(np.arange(n))
    for cls in ("nan_start", "zero_length", "nan_end"):
        assert (ref[c == M.SEG_CLASSES.index(cls)] == 1.0).all(), cls
    wd, p, org, d, t, obj = M.closest_hit_case(oracle, name, 0, {}, 41, n)
    print(name, "objects", np.unique(obj, return_counts=True))
    assert len(np.unique(obj)) >= 3
    c = M.ray_class(np.arange(n))
    miss_t = np.unique(t[~np.isnan(t) & (obj == 0xFFFFFFFF)])  # what a ray that hits nothing reports: t_max, beyond every hit
    assert len(miss_t) == 1 and miss_t[0] > t[obj != 0xFFFFFFFF].max()
    for cls in ("nan_origin", "nan_dir"):
        k = c == M.RAY_CLASSES.index(cls)
        assert (obj[k] == 0xFFFFFFFF).all() and (np.isnan(t[k]) | (t[k] == miss_t[0])).all(), cls
    assert M.same_t(t, t).all() and not M.same_t(t[:1000], t[1:1001]).all()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513])
def test_generators_and_oracle_helpers_at_the_queue_edge_sizes(oracle, n):
    """The sizes of test_extend_queue_edges / test_shadow_queue_edges: the generators and the cached oracle cases take them (fewer entries than oracle threads,
    than a class period, than a chunk) and return arrays of length n that equal the plain oracle calls."""
    a, b = M.segments(n, 31)
    org, d = M.rays(n, 41)
    assert a.shape == b.shape == org.shape == d.shape == (n, 3)
    assert np.array_equal(M.seg_class(np.arange(n)), M.seg_class(np.arange(513))[:n])
    for name in ("s1", "bulb", "two_sdfs"):
        wd, p, ca, cb, ref = M.occluded_case(oracle, name, {}, 31, n)
        assert ca is a and cb is b and ref.shape == (n,) and ref.dtype == np.float32
        assert np.array_equal(ref, oracle.test_occluded(wd, p, a, b))
        ev, it = M.occluded_counts(name, {}, 31, n)
        assert ev >= n and it >= 0  # every segment is evaluated at least once
    for name in ("s1", "bulb"):
        wd, p, co, cd, t, obj = M.closest_hit_case(oracle, name, 0, {}, 41, n)
        assert co is org and cd is d and t.shape == obj.shape == (n,)
        rt, robj = oracle.closest_hit(wd, p, 0, org, d)
        assert np.array_equal(obj, robj) and M.same_t(t, rt).all()
