"""numpy restatement of the HDR display transform of the Color channel (rayn_hip_display_pixels_device / rayn_hip_display_color_device,
include/rayn_hip.h): metering with its fixed summation order, adaptation, bloom pyramid, tone operators and save_to's output chain,
operation by operation in float32, so that the tests can compare the kernels with it bit for bit.  logf / expf are the pinned dm_logf /
dm_expf of include/rayn_detmath.h, evaluated by the oracle (oracle_detmath ops 6 and 0); gamma goes through image.gamma_corrected.
dtype=np.float64 reads the same formulas in float64 with numpy's log / exp (a cross-check of the float32 reading, not bit-exact)."""
import numpy as np

from rayn_amd import image

TONE_LINEAR, TONE_REINHARD, TONE_ACES = 0, 1, 2
# Wrong readings, for tests/post_edge_cases.py (mutant=None: the definition's bits).  meter_ge0: a pixel is metered when l >= 0;
# no_floor: the logarithm of l itself, without the 1e-4 floor; adapt_always_blend: m_prev + (m_now - m_prev) adapt whatever valid and
# adapt are; quant_round: the 8-bit value is rounded to nearest instead of truncated;
# bright_fin_after: the bright pass tests e c, not c, for finiteness.
MUTANTS = ("meter_ge0", "no_floor", "adapt_always_blend", "quant_round", "bright_fin_after")
# reinhard_ge0 (the operator is on when lx >= 0): at lx = +0 or -0.0 the scale is (1 + lx iw2) / (1 + lx) = 1 / 1 = 1.0f exactly, and
# v * 1.0f has v's bits (a NaN's payload aside): the reading changes no bit.
EQUIVALENT = ("reinhard_ge0",)


def _oracle(op, x):
    from oracle import oracle_py
    return oracle_py.detmath(op, np.ascontiguousarray(x, np.float32).reshape(-1)).reshape(np.shape(x))


def _logf(x, f):
    return _oracle(6, x) if f is np.float32 else np.log(x)


def _expf(x, f):
    return _oracle(0, x) if f is np.float32 else np.exp(x)


def _rmax(a, b):
    """Rust's f32::max: a NaN operand yields the other one (dtype-preserving, unlike image._rust_max)."""
    return np.where(np.isnan(a), b, np.where(np.isnan(b), a, np.maximum(a, b)))


def luminance(c, f):
    return (f(0.2126) * c[..., 0] + f(0.7152) * c[..., 1]) + f(0.0722) * c[..., 2]


def fin0(c):
    return np.where(np.isfinite(c), c, c.dtype.type(0))


def halving_tree(a):
    """a[j] += a[j + s] for s = 128, 64, ..., 1 over the last axis (256 long); returns a[0].  The dtype is the array's."""
    s = a.shape[-1] // 2
    while s >= 1:
        a = a[..., :s] + a[..., s:2 * s]
        s //= 2
    return a[..., 0]


def input_color(color, background, transparent_background, f=np.float32):
    """c as (n, 3): color + background in the Color + Background arm (the sum in float32, as the film's channels are), else color."""
    c = np.asarray(color, np.float32).reshape(-1, 3)
    if background is not None and not transparent_background:
        with np.errstate(all="ignore"):
            c = c + np.asarray(background, np.float32).reshape(-1, 3)
    return c.astype(f)


def meter(c, f=np.float32, mutant=None):
    """(S, N) of the two-stage sum over the film pixels c (n, 3)."""
    n = len(c)
    with np.errstate(all="ignore"):
        l = luminance(c, f)
        ok = np.isfinite(c).all(-1) & ((l >= 0) if mutant == "meter_ge0" else (l > 0))
        floored = np.where(ok, l, f(1)) if mutant == "no_floor" else _rmax(np.where(ok, l, f(1)), f(1e-4))
        v = np.where(ok, _logf(floored.astype(f), f).astype(f), f(0))
        nb = (n + 255) // 256
        pv, pk = np.zeros(nb * 256, f), np.zeros(nb * 256, np.uint32)
        pv[:n], pk[:n] = v, ok
        part_v, part_k = halving_tree(pv.reshape(nb, 256)), halving_tree(pk.reshape(nb, 256))
        rows = (nb + 255) // 256
        qv, qk = np.zeros(rows * 256, f), np.zeros(rows * 256, np.uint32)
        qv[:nb], qk[:nb] = part_v, part_k
        acc_v, acc_k = np.zeros(256, f), np.zeros(256, np.uint32)
        for r in range(rows):  # accumulator t: the partials t, t + 256, ... in ascending order, starting from 0
            acc_v = acc_v + qv[r * 256:(r + 1) * 256]
            acc_k = acc_k + qk[r * 256:(r + 1) * 256]
        return halving_tree(acc_v), int(halving_tree(acc_k))


def expose(c, p, state, f=np.float32, mutant=None):
    """(e, new state (m, valid)) for the input colour c under the parameters p (a rayn_display_params) and the state before."""
    if not p.auto_exposure:
        return f(np.float32(p.exposure_scale)), state
    S, N = meter(c, f, mutant)
    m_prev, valid = f(state[0]), int(state[1])
    if N == 0:
        return f(1), state
    key, adapt = f(np.float32(p.key)), f(np.float32(p.adapt))
    with np.errstate(all="ignore"):
        m_now = S / f(np.float32(N))
        m = m_now if (valid == 0 or adapt == 1) and mutant != "adapt_always_blend" else m_prev + (m_now - m_prev) * adapt
        e = key / f(_expf(np.array([m], f), f)[0])
    return f(e), (f(m), 1)


def level_sizes(w, h, levels):
    out = [(w, h)]
    for _ in range(levels):
        w, h = (w + 1) // 2, (h + 1) // 2
        out.append((w, h))
    return out


def downsample(d, f):
    hp, wp = d.shape[:2]
    w, h = (wp + 1) // 2, (hp + 1) // 2
    x0, y0 = 2 * np.arange(w), 2 * np.arange(h)
    x1, y1 = np.minimum(x0 + 1, wp - 1), np.minimum(y0 + 1, hp - 1)
    A, B, C, D = d[y0][:, x0], d[y0][:, x1], d[y1][:, x0], d[y1][:, x1]
    return ((A + B) + (C + D)) * f(0.25)


def _up_axis(n, ns, f):
    x = np.arange(n)
    half, odd = x // 2, (x & 1) == 1
    t0 = np.where(odd, half, half - 1)
    t1 = np.where(odd, half + 1, half)
    w0 = np.where(odd, f(0.75), f(0.25)).astype(f)
    w1 = np.where(odd, f(0.25), f(0.75)).astype(f)
    return np.clip(t0, 0, ns - 1), np.clip(t1, 0, ns - 1), w0, w1


def upsample(u, w, h, f):
    """The bilinear 2x filter of u (hs, ws, 3) at the w x h pixels of the level below."""
    hs, ws = u.shape[:2]
    x0, x1, wx0, wx1 = _up_axis(w, ws, f)
    y0, y1, wy0, wy1 = _up_axis(h, hs, f)
    a, b, c, d = u[y0][:, x0], u[y0][:, x1], u[y1][:, x0], u[y1][:, x1]
    wx0, wx1 = wx0[None, :, None], wx1[None, :, None]
    wy0, wy1 = wy0[:, None, None], wy1[:, None, None]
    return wy0 * (wx0 * a + wx1 * b) + wy1 * (wx0 * c + wx1 * d)


def bloom(c, e, width, height, levels, threshold, strength, f=np.float32, mutant=None):
    """The bloom plane B at level 0, (n, 3) in film order."""
    w, h, L = int(width), int(height), int(levels)
    with np.errstate(all="ignore"):
        ec = fin0((e * c).astype(f)) if mutant == "bright_fin_after" else e * fin0(c)
        D = [_rmax(ec - f(np.float32(threshold)), f(0)).astype(f).reshape(h, w, 3)]
        for _ in range(L):
            D.append(downsample(D[-1], f))
        U = D[L]
        for k in range(L - 1, -1, -1):
            hk, wk = D[k].shape[:2]
            U = D[k] + upsample(U, wk, hk, f)
        scale = f(np.float32(strength)) / f(np.float32(L + 1))
        return (U * scale).reshape(-1, 3)


def tone(x, kind, iw2, f=np.float32, mutant=None):
    with np.errstate(all="ignore"):
        if kind == TONE_REINHARD:
            lx = luminance(x, f)
            on = np.isfinite(lx) & ((lx >= 0) if mutant == "reinhard_ge0" else (lx > 0))
            s = (f(1) + lx * f(np.float32(iw2))) / (f(1) + lx)
            return np.where(on[..., None], x * s[..., None], x)
        if kind == TONE_ACES:
            y = _rmax(x, f(0)).astype(f)
            return (y * (f(2.51) * y + f(0.03))) / (y * (f(2.43) * y + f(0.59)) + f(0.14))
        return x


def _quant_round(x):
    """the quant_round reading of image._quant"""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.asarray(x, np.float32) * np.float32(255.0)
        return np.floor(image._rust_max(image._rust_min(v, np.float32(255.0)), np.float32(0.0)) + np.float32(0.5)).astype(np.uint8)


def display(color, width, height, p, background=None, alpha=None, transparent_background=False, state=(0.0, 0), dtype=np.float32, mutant=None):
    """The whole transform of a film (color / background (n, 3), alpha (n,), film order) under the rayn_display_params p.  Returns a dict:
    d (n, 3) the float plane in film order, e, m (the state's after the call; 0 with manual exposure), state (m, valid), bloom (n, 3) or
    None, and - in float32 only - image, the 8-bit image (h, w, 3 or 4), rows top-down."""
    f = np.dtype(dtype).type
    w, h = int(width), int(height)
    if transparent_background and alpha is None:
        raise ValueError("Attempted to write Color channel with insufficient channels")
    c = input_color(color, background, transparent_background, f)
    e, state = expose(c, p, state, f, mutant)
    with np.errstate(all="ignore"):
        x = e * c
        B = None
        if p.levels:
            B = bloom(c, e, w, h, p.levels, p.threshold, p.strength, f, mutant)
            x = x + B
        d = tone(x, p.tone, p.iw2, f, mutant).astype(f)
    out = {"d": d, "e": e, "m": f(state[0]) if p.auto_exposure else f(0), "state": state, "bloom": B, "image": None}
    if f is np.float32:
        dd = d.reshape(h, w, 3)
        quant = _quant_round if mutant == "quant_round" else image._quant
        if transparent_background:
            rgb = quant(image.gamma_corrected(image.saturated(dd)))
            out["image"] = np.concatenate([rgb, quant(np.asarray(alpha, np.float32).reshape(h, w))[..., None]], axis=-1)[::-1]
        elif background is not None:
            out["image"] = quant(image.gamma_corrected(image.saturated(dd)))[::-1]
        else:
            out["image"] = quant(image.gamma_corrected(dd))[::-1]
    return out
