"""Numpy restatement of progressive rendering (include/rayn_hip.h, "progressive rendering"), f32 operation by f32
operation, and of the whole loop around a pluggable `render_epoch(seed, tile_subset) -> film` callable.  With the CPU oracle as that
callable it is the CPU reference of the feature.  Written from the definition alone: it imports nothing from rayn_amd.

A film is a dict of float32 arrays color (n, 3), alpha (n), background (n, 3), normal (n, 3) in film pixel order (x + y * width)."""
import numpy as np

F32 = np.float32
STRIDE = 65536
# Wrong readings of the definition, for tests/post_edge_cases.py (mutant=None: the definition's bits).  e_ge: an outlier is e >= target;
# retire_lt: outliers * 1000 < permille * pixels; epochs_gt: n > min_epochs; percent: permille read as percent; u32_products: both
# products of the retirement rule in 32 bits; nominal_tile_pixels: tile_w * tile_h in place of the clipped tile's pixels; fnn_u32:
# n (n - 1) in 32 bits before the conversion; compact_no_carry: the compaction forgets the chunks before (PN.compact only).
MUTANTS = ("e_ge", "retire_lt", "epochs_gt", "percent", "u32_products", "nominal_tile_pixels", "fnn_u32", "compact_no_carry")
# maxe_ge (max_e over e >= 0 in place of e > 0, by bit pattern as the kernel takes it) differs only for e = -0.0, whose pattern is
# 0x80000000.  e = se / (|mean_y| + noise_floor): the divisor is |mean_y| (+0 or positive) plus a noise_floor that is >= 0 or -0.0, and
# +0 + -0 = +0, so it is never -0 or negative; se = sqrt(m2 / fnn) is -0 only for m2 = -0.0, and m2 starts at +0 (the reset) and becomes
# m2 + d (y - mean), a sum that is -0 only when BOTH terms are -0: by induction m2 is never -0.  A negative m2 gives a NaN.  So e is NaN,
# +0 or positive: the reading is equivalent on every state the reset entry started.
EQUIVALENT = ("maxe_ge",)
CHUNK = 1024  # tiles per trip of the compaction
FILM_KEYS = ("color", "alpha", "background", "normal")


def seed(frame, epoch, max_bounces, volume_marches):
    """f + e * 65536; an error where the sets of one epoch number more than the stride or the seed does not fit 32 bits."""
    sets = 3 + (max_bounces + 1) * (15 + 9 * volume_marches)
    s = frame + epoch * STRIDE
    if sets > STRIDE or s >= 1 << 32:
        raise ValueError("no epoch seed")
    return s


def tile_rects(width, height, tw, th):
    """the reference's tile list (src/film.rs:399-427): x-major, (res + res % tile) / tile tiles per axis"""
    nx, ny = (width + width % tw) // tw, (height + height % th) // th
    return [(tx * tw, ty * th, min(tx * tw + tw, width), min(ty * th + th, height)) for tx in range(nx) for ty in range(ny)]


def flat(film):
    return {"color": np.array(film["color"], F32).reshape(-1, 3), "alpha": np.array(film["alpha"], F32).reshape(-1),
            "background": np.array(film["background"], F32).reshape(-1, 3), "normal": np.array(film["normal"], F32).reshape(-1, 3)}


class State:
    def __init__(self, width, height, tile_size):
        self.width, self.height, self.tile_size = width, height, tuple(tile_size)
        self.rects = tile_rects(width, height, *self.tile_size)
        n, t = width * height, len(self.rects)
        # -0.0 is the identity of IEEE addition: the first epoch's sums are the epoch film's bits
        self.sum = {"color": np.full((n, 3), -0.0, F32), "alpha": np.full(n, -0.0, F32), "background": np.full((n, 3), -0.0, F32),
                    "normal": np.full((n, 3), -0.0, F32)}
        self.mean_y, self.m2 = np.zeros(n, F32), np.zeros(n, F32)
        self.epochs, self.retired, self.outliers = np.zeros(t, np.uint32), np.zeros(t, np.uint32), np.zeros(t, np.uint32)
        self.max_e = np.zeros(t, F32)
        self.mean = {"color": np.zeros((n, 3), F32), "alpha": np.zeros(n, F32), "background": np.zeros((n, 3), F32), "normal": np.zeros((n, 3), F32)}

    def pixels_of(self, k):
        x0, y0, x1, y1 = self.rects[k]
        ys, xs = np.mgrid[y0:y1, x0:x1]
        return (xs + ys * self.width).reshape(-1)

    def active(self):
        return np.flatnonzero(self.retired == 0).astype(np.uint32)

    def totals(self):
        return {"active_tiles": int((self.retired == 0).sum()), "max_e": float(self.max_e.max(initial=F32(0))),
                "outlier_pixels": int(self.outliers.astype(np.uint64).sum())}


def e_p(mean_y, m2, n, noise_floor, mutant=None):
    """se / (|mean_y| + noise_floor) per pixel in f32; n >= 2.  n (n - 1) is an exact integer, rounded once to f32."""
    nn = n * (n - 1)
    if mutant == "fnn_u32":
        nn &= 0xFFFFFFFF
    with np.errstate(all="ignore"):
        se = np.sqrt(m2 / F32(nn))
        return (se / (np.abs(mean_y) + F32(noise_floor))).astype(F32)


def tile_report(e, target_error, mutant=None):
    """(outliers, max_e) of one tile's e_p: a NaN is neither an outlier nor a maximum; both are independent of the order of e"""
    with np.errstate(invalid="ignore"):
        outliers = int(((e >= F32(target_error)) if mutant == "e_ge" else (e > F32(target_error))).sum())
        pos = e[e > 0]
        if mutant == "maxe_ge":  # the largest bit pattern, as the kernel takes the maximum
            pos = np.ascontiguousarray(e[e >= 0]).view(np.uint32)
            return outliers, (F32(0) if not pos.size else np.array([pos.max()], np.uint32).view(F32)[0])
    return outliers, (pos.max() if pos.size else F32(0))


def retires(n, outliers, tile_pixels, min_epochs, outlier_permille, mutant=None):
    if not (n > min_epochs if mutant == "epochs_gt" else n >= min_epochs):
        return False
    lhs, rhs = outliers * (100 if mutant == "percent" else 1000), outlier_permille * tile_pixels  # Python integers: exact
    if mutant == "u32_products":
        lhs, rhs = lhs & 0xFFFFFFFF, rhs & 0xFFFFFFFF
    return lhs < rhs if mutant == "retire_lt" else lhs <= rhs


def compact(retired, mutant=None):
    """(the active list, its length) as the compaction builds them, CHUNK tile records at a time, each chunk's active tiles appended behind
    those of the chunks before; list entries it never writes are -1.  Without a mutant: flatnonzero(retired == 0) and its length."""
    retired = np.asarray(retired)
    out, run = np.full(len(retired), -1, np.int64), 0
    for base in range(0, len(retired), CHUNK):
        act = base + np.flatnonzero(retired[base:base + CHUNK] == 0)
        if mutant == "compact_no_carry":
            run = 0
        out[run:run + len(act)] = act
        run += len(act)
    return out, run


def accumulate(state, film, tiles=None, target_error=0.05, noise_floor=0.05, min_epochs=4, outlier_permille=50, adaptive=True, mutant=None):
    """One epoch film into the listed tiles (ascending; None = all) of the state; updates state.mean for those tiles."""
    film = flat(film)
    tiles = range(len(state.rects)) if tiles is None else [int(k) for k in tiles]
    assert all(b > a for a, b in zip(tiles, tiles[1:])) and all(0 <= k < len(state.rects) for k in tiles)
    with np.errstate(all="ignore"):
        for k in tiles:
            px = state.pixels_of(k)
            n = int(state.epochs[k]) + 1
            fn = F32(n)
            for key in FILM_KEYS:
                state.sum[key][px] = state.sum[key][px] + film[key][px]
                state.mean[key][px] = state.sum[key][px] / fn
            c = film["color"][px] + film["background"][px]
            y = (F32(0.2126) * c[:, 0] + F32(0.7152) * c[:, 1]) + F32(0.0722) * c[:, 2]
            d = y - state.mean_y[px]
            mean = state.mean_y[px] + d / fn
            state.m2[px] = state.m2[px] + d * (y - mean)
            state.mean_y[px] = mean
            state.epochs[k] = n
            if n >= 2:
                state.outliers[k], state.max_e[k] = tile_report(e_p(state.mean_y[px], state.m2[px], n, noise_floor, mutant), target_error, mutant)
            else:
                state.outliers[k], state.max_e[k] = 0, F32(0)
            pixels = state.tile_size[0] * state.tile_size[1] if mutant == "nominal_tile_pixels" else len(px)
            if adaptive and retires(n, int(state.outliers[k]), pixels, min_epochs, outlier_permille, mutant):
                state.retired[k] = 1
    return state


def run(render_epoch, width, height, tile_size, frame, max_bounces, volume_marches, target_error=0.05, noise_floor=0.05, min_epochs=4,
        max_epochs=64, outlier_permille=50, adaptive=True, state=None, first_epoch=0, on_epoch=None):
    """The loop: epoch e renders the active tiles under seed(frame, e) and is accumulated; ends when no tile is active or after max_epochs.
    Returns (state, history): history[i] = (seed, rendered tile list or None for all, active list after the epoch)."""
    state = State(width, height, tile_size) if state is None else state
    history = []
    epoch = first_epoch
    active = state.active()
    while epoch < max_epochs and len(active):
        s = seed(frame, epoch, max_bounces, volume_marches)
        subset = None if len(active) == len(state.rects) else active
        film = render_epoch(s, subset)
        accumulate(state, film, subset, target_error, noise_floor, min_epochs, outlier_permille, adaptive)
        active = state.active()
        history.append((s, subset, active))
        epoch += 1
        if on_epoch is not None and on_epoch(state, history) is False:
            break
    return state, history
