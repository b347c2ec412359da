"""Operands and the IEEE reference for div3_by (rayn_amd/csrc/device_core.h): v / m as three binary32 divisions by one denominator.
Shared by the device probe test (test_div3_device.py) and its numpy twin (test_div3.py)."""
import numpy as np

LO, HI = np.float32(2.0 ** -60), np.float32(2.0 ** 60)  # the window [2^-60, 2^60) of the denominator and of every |component|
LO_BITS, HI_BITS = 0x21800000, 0x5D800000


def _nx(x, up):
    x = np.float32(x)
    return np.nextafter(x, np.float32(np.inf) if up else np.float32(-np.inf), dtype=np.float32)


def operands(n_bulk=1 << 22, seed=17):
    """(v [n, 3], m [n]) float32: the edge cases first, then a seeded bulk, log-uniform in exponent."""
    f32 = np.float32
    tiny, huge = f32(2.0 ** -126), np.finfo(np.float32).max
    den = [LO, _nx(LO, False), _nx(LO, True), HI, _nx(HI, False), _nx(HI, True), f32(1.0), f32(3.0), f32(1.9999999), f32(2.0 ** 59), f32(2.0 ** -59),
           f32(2.0 ** 30 * 1.3), f32(2.0 ** -30 * 1.7), -LO, -HI, f32(-1.5), f32(0.0), f32(-0.0), f32(np.inf), f32(-np.inf), f32(np.nan), f32(1e-40), f32(-1e-42), tiny, huge]
    num = [LO, _nx(LO, False), _nx(LO, True), HI, _nx(HI, False), _nx(HI, True), f32(1.0), f32(-1.0), f32(1.5), f32(0.1), f32(-7.0),
           f32(0.0), f32(-0.0), f32(1e-40), f32(-1e-45), tiny, -tiny, huge, -huge, f32(np.inf), f32(-np.inf), f32(np.nan),
           # quotients at the ends of the normal range: with m = 2^59 the numerators 2^-67, just below (denormal quotient) and with m = 2^-60 the numerators
           # 2^67 x 1.99.. (largest normal), 2^68 (overflow); with m = 2^-59 the numerator 2^59 (2^118, inside), with m = 2^59 the numerator 2^-60 (2^-119, inside)
           f32(2.0 ** -67), _nx(f32(2.0 ** -67), False), f32(2.0 ** -68), _nx(f32(2.0 ** 68), False), f32(2.0 ** 68), f32(2.0 ** 100), f32(2.0 ** -100),
           f32(2.0 ** 59), f32(-(2.0 ** 59) * 1.1), f32(2.0 ** -59 * 1.3)]
    den, num = np.array(den, np.float32), np.array(num, np.float32)
    # every (numerator, denominator) pair in every component position, next to two ordinary components
    nn, dd = np.meshgrid(num, den, indexing="ij")
    nn, dd = nn.ravel(), dd.ravel()
    grid_v = np.concatenate([np.stack(np.roll([nn, np.full_like(nn, 1.5), -nn], s, axis=0), 1) for s in range(3)])
    grid_m = np.tile(dd, 3)
    rng = np.random.default_rng(seed)
    # random triples of the special numerators over random special denominators
    k = 1 << 17
    mix_v = num[rng.integers(0, num.size, (k, 3))]
    mix_m = den[rng.integers(0, den.size, k)]
    # bulk: exponents -64 .. 63 (three quarters of the triples fall inside the window), random signs on the components, one denominator in 16 negative
    e = rng.integers(-64, 64, (n_bulk, 4)).astype(np.float64)
    x = rng.uniform(1.0, 2.0, (n_bulk, 4)) * np.exp2(e)
    x[:, :3] *= rng.choice([-1.0, 1.0], (n_bulk, 3))
    x[rng.integers(0, 16, n_bulk) == 0, 3] *= -1.0
    x = x.astype(np.float32)
    # a slice of near-equal operands (quotients next to 1, where the correction steps decide the last bit) and one with exact quotients
    s = slice(0, n_bulk // 16)
    x[s, 0] = x[s, 3] * rng.uniform(0.999999, 1.000001, s.stop).astype(np.float32)
    s2 = slice(n_bulk // 16, n_bulk // 8)
    x[s2, 1] = x[s2, 3] * rng.integers(1, 1 << 12, s2.stop - s2.start).astype(np.float32)
    v = np.ascontiguousarray(np.concatenate([grid_v, mix_v, x[:, :3]]), np.float32)
    m = np.ascontiguousarray(np.concatenate([grid_m, mix_m, x[:, 3]]), np.float32)
    return v, m


def in_window(v, m):
    """the lanes div3_by serves with the shared reciprocal (everything else runs the literal divisions)"""
    a = v.view(np.uint32) & np.uint32(0x7FFFFFFF)
    mb = m.view(np.uint32)
    return (a.min(1) >= LO_BITS) & (a.max(1) < HI_BITS) & (mb >= LO_BITS) & (mb < HI_BITS) & ((mb & np.uint32(0x7FFFFF)) != 0x7FFFFF)


def ieee(v, m):
    with np.errstate(all="ignore"):
        return (v / m[:, None]).astype(np.float32)


def mismatches(got, ref):
    """indices where the bits differ; two NaNs are equal whatever their payload (IEEE 754 leaves it open)"""
    got, ref = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(ref, np.float32)
    bad = (got.view(np.int32) != ref.view(np.int32)) & ~(np.isnan(got) & np.isnan(ref))
    return np.argwhere(bad)
