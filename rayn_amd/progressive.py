"""Host side of progressive rendering (rayn_hip_progressive_*, include/rayn_hip.h; an extension: rayn only carries an unused
progressive_epoch counter): the `Progressive` parameters, the epoch seed, the layout of the device state as numpy arrays, the error map and
sample-count image made from it, and the checkpoint file.  Everything here works on numpy arrays and needs no GPU."""
import ctypes as C
import dataclasses

import numpy as np

from ._lib import lib

SEED_STRIDE = 65536  # seed(f, e) = f + e * SEED_STRIDE


@dataclasses.dataclass(frozen=True)
class Progressive:
    """Parameters of Film.render_progressive.  A pixel's error estimate is e_p = se / (|mean_y| + noise_floor), se the standard error of
    the mean of its luminance over the epochs; a pixel with e_p > `target_error` is an outlier; a tile retires once it has `min_epochs`
    (>= 2) epochs and at most `outlier_permille` per thousand of its pixels are outliers; the render ends when every tile has retired
    or after `max_epochs` (<= 65536).  `adaptive=False` retires nothing: every epoch renders the whole frame.  Stopping on an estimate
    of the error biases the mean slightly (the adaptive-sampling bias); `min_epochs` bounds it.

    The defaults were chosen on the shipped scene (rayn_amd.setup at 1280x720, SAMPLES = 2, i.e. 8 spp per epoch, max_epochs 64; DESIGN.md
    section 8) among six candidates, by the MSE of the saturated Color + Background (against 256 non-adaptive epochs) relative to that of
    a non-adaptive render of the same path count: target 0.05 with a floor of 0.05 (so that the near-black cavities are not chased for
    ever), 50 permille of a tile's pixels allowed above it (silhouette pixels converge last and would hold a whole tile open) and 4
    epochs before a tile may retire gave 0.59x; a target of 0.1 or 0.03, a floor of 0.01 and 10 permille all did worse (0.74 - 0.87x)."""
    target_error: float = 0.05
    min_epochs: int = 4
    max_epochs: int = 64
    outlier_permille: int = 50
    noise_floor: float = 0.05
    adaptive: bool = True

    def __post_init__(self):
        for name in ("min_epochs", "max_epochs", "outlier_permille"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Progressive.{name} must be an int, got {v!r}")
        if self.min_epochs < 2:
            raise ValueError(f"Progressive.min_epochs must be >= 2, got {self.min_epochs!r}")
        if not self.min_epochs <= self.max_epochs <= SEED_STRIDE:
            raise ValueError(f"Progressive.max_epochs must be in min_epochs..{SEED_STRIDE}, got {self.max_epochs!r}")
        if not 0 <= self.outlier_permille <= 1000:
            raise ValueError(f"Progressive.outlier_permille must be in 0..1000, got {self.outlier_permille!r}")
        for name in ("target_error", "noise_floor"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.floating, np.integer)):
                raise ValueError(f"Progressive.{name} must be a number, got {v!r}")
            f = float(v)  # the C entry takes it as an f32: check that value too
            with np.errstate(over="ignore"):
                f32 = float(np.float32(f))
            if not (0.0 <= f < float("inf") and f32 < float("inf")):
                raise ValueError(f"Progressive.{name} must be finite and >= 0, got {v!r}")
        if not isinstance(self.adaptive, (bool, np.bool_)):
            raise ValueError(f"Progressive.adaptive must be a bool, got {self.adaptive!r}")

    def to_abi(self):
        from . import _abi
        return _abi.ProgressiveParams(float(self.target_error), float(self.noise_floor), int(self.min_epochs), int(self.max_epochs),
                                      int(self.outlier_permille), int(bool(self.adaptive)))


def progressive_seed(frame, epoch, max_bounces, volume_marches):
    """rayn_progressive_seed: the sample-table offset of epoch `epoch` of frame `frame`, frame + epoch * 65536 (epoch 0 is the plain
    frame).  ValueError where the sets of one epoch would reach into the next epoch's or the seed would not fit 32 bits."""
    out = C.c_uint32()
    for name, v in (("frame", frame), ("epoch", epoch), ("max_bounces", max_bounces), ("volume_marches", volume_marches)):
        if not 0 <= int(v) < 1 << 32:
            raise ValueError(f"progressive_seed: {name} = {v!r} does not fit 32 bits")
    if lib().rayn_progressive_seed(int(frame), int(epoch), int(max_bounces), int(volume_marches), C.byref(out)) != 0:
        raise ValueError(f"no epoch seed for frame {frame}, epoch {epoch}, {max_bounces} bounces, {volume_marches} volume marches: "
                         f"more than {SEED_STRIDE} sample sets per epoch, or frame + epoch * {SEED_STRIDE} >= 2^32")
    return out.value


def state_bytes(width, height, tile_size):
    """rayn_progressive_state_bytes: bytes of device state of a width x height film cut into tile_size tiles (0 for a rejected geometry)."""
    return int(lib().rayn_progressive_state_bytes(int(width), int(height), int(tile_size[0]), int(tile_size[1])))


def tile_rects(width, height, tile_size):
    """(x0, y0, x1, y1) of every tile in the reference's order (x-major, src/film.rs:399-427, incl. its under-coverage quirk)."""
    tw, th = int(tile_size[0]), int(tile_size[1])
    nx, ny = (width + width % tw) // tw, (height + height % th) // th
    return [(tx * tw, ty * th, min(tx * tw + tw, width), min(ty * th + th, height)) for tx in range(nx) for ty in range(ny)]


def split_state(raw, width, height, tile_size):
    """The device state (a uint8 array of state_bytes) as named numpy arrays: the running sums in the film's layout, mean_y, m2, the tile
    records and the active list."""
    raw = np.ascontiguousarray(raw, np.uint8).reshape(-1)
    n, t = width * height, len(tile_rects(width, height, tile_size))
    if raw.size != state_bytes(width, height, tile_size):
        raise ValueError(f"a state of {raw.size} bytes is not that of a {width}x{height} film with {tile_size[0]}x{tile_size[1]} tiles")
    planes = raw[: 48 * n].view(np.float32).reshape(3, n, 4)
    rec = raw[48 * n: 48 * n + 16 * t].view(np.uint32).reshape(t, 4)
    totals = raw[48 * n + 16 * t: 48 * n + 16 * t + 16].view(np.uint32)
    active = raw[48 * n + 16 * t + 16: 48 * n + 20 * t + 16].view(np.uint32)
    return {"sum_color": planes[0, :, :3].copy(), "sum_alpha": planes[0, :, 3].copy(), "sum_background": planes[1, :, :3].copy(),
            "mean_y": planes[1, :, 3].copy(), "sum_normal": planes[2, :, :3].copy(), "m2": planes[2, :, 3].copy(),
            "epochs": rec[:, 0].copy(), "retired": rec[:, 1].copy(), "outliers": rec[:, 2].copy(), "max_e": rec[:, 3].copy().view(np.float32),
            "active": active[: int(totals[0])].copy()}


def join_state(arrays, width, height, tile_size):
    """The inverse of split_state: the device state as a uint8 array (the totals are taken again from the records)."""
    n, t = width * height, len(tile_rects(width, height, tile_size))
    raw = np.zeros(state_bytes(width, height, tile_size), np.uint8)
    planes = raw[: 48 * n].view(np.float32).reshape(3, n, 4)
    for i, (vec, scalar) in enumerate((("sum_color", "sum_alpha"), ("sum_background", "mean_y"), ("sum_normal", "m2"))):
        planes[i, :, :3] = np.asarray(arrays[vec], np.float32).reshape(n, 3)
        planes[i, :, 3] = np.asarray(arrays[scalar], np.float32).reshape(n)
    rec = raw[48 * n: 48 * n + 16 * t].view(np.uint32).reshape(t, 4)
    for i, name in enumerate(("epochs", "retired", "outliers")):
        rec[:, i] = np.asarray(arrays[name], np.uint32).reshape(t)
    rec[:, 3] = np.ascontiguousarray(arrays["max_e"], np.float32).reshape(t).view(np.uint32)
    active = np.flatnonzero(rec[:, 1] == 0).astype(np.uint32)
    totals = raw[48 * n + 16 * t: 48 * n + 16 * t + 16].view(np.uint32)
    outliers = int(rec[:, 2].astype(np.uint64).sum())
    totals[:] = (len(active), int(rec[:, 3].max(initial=0)), outliers & 0xFFFFFFFF, outliers >> 32)
    raw[48 * n + 16 * t + 16: 48 * n + 20 * t + 16].view(np.uint32)[: len(active)] = active
    return raw


def _per_pixel(per_tile, width, height, tile_size, fill=0):
    out = np.full((height, width), fill, np.asarray(per_tile).dtype)
    for v, (x0, y0, x1, y1) in zip(per_tile, tile_rects(width, height, tile_size)):
        out[y0:y1, x0:x1] = v
    return out


def mean_film(arrays, width, height, tile_size):
    """The mean film of a state, sum / (float)n per tile in f32 - the bits the accumulate kernel wrote (film layout, bottom-up rows).
    Pixels of tiles without an epoch, and those the tiles do not cover, are 0."""
    n = _per_pixel(arrays["epochs"], width, height, tile_size).reshape(-1)
    fn = np.maximum(n, 1).astype(np.float32)
    out = {}
    with np.errstate(all="ignore"):
        for key in ("color", "alpha", "background", "normal"):
            s = np.asarray(arrays["sum_" + key], np.float32)
            m = s / (fn[:, None] if s.ndim == 2 else fn)
            m[n == 0] = 0.0
            out[key] = m.astype(np.float32)
    return out


def error_map(arrays, width, height, tile_size, noise_floor):
    """e_p = sqrtf(m2 / (float)(n (n - 1))) / (fabsf(mean_y) + noise_floor) of every pixel in f32 ((height, width), bottom-up rows like the
    film); 0 where the pixel's tile has fewer than two epochs."""
    n = _per_pixel(arrays["epochs"].astype(np.uint64), width, height, tile_size).reshape(-1)
    with np.errstate(all="ignore"):
        fnn = np.maximum(n * (n - np.minimum(n, 1)), 1).astype(np.float32)
        se = np.sqrt(np.asarray(arrays["m2"], np.float32) / fnn)
        e = se / (np.abs(np.asarray(arrays["mean_y"], np.float32)) + np.float32(noise_floor))
    e[n < 2] = 0.0
    return e.astype(np.float32).reshape(height, width)


def sample_count_image(epochs, width, height, tile_size):
    """u8 heat map of the per-tile epoch counts, rows top-down: 255 = the largest count, 0 = no epoch (or outside every tile)."""
    epochs = np.asarray(epochs, np.uint64)
    top = max(int(epochs.max(initial=0)), 1)
    img = _per_pixel(((epochs * 255 + top // 2) // top).astype(np.uint8), width, height, tile_size)
    return img[::-1].copy()


# ---- checkpoint file -------------------------------------------------------------------------------------------------------------

KEY_FIELDS = ("resolution", "tile_size", "samples", "max_bounces", "volume_marches", "frame", "time_range", "filter", "world",
              "target_error", "noise_floor", "min_epochs", "outlier_permille", "adaptive", "fma_policy")
STATE_FIELDS = ("sum_color", "sum_alpha", "sum_background", "sum_normal", "mean_y", "m2", "epochs", "retired", "outliers", "max_e")


def checkpoint_key(resolution, tile_size, samples, max_bounces, volume_marches, frame, time_range, filter, world_bytes, progressive, fma_policy):
    """What a checkpoint belongs to: everything that decides the epochs' films and the retirement (max_epochs does not)."""
    fk, fr = (0, 1.5) if filter is None else (filter.kind, filter.radius)
    fp = getattr(filter, "params", (0.0, 0.0))
    return {"resolution": np.asarray(resolution, np.uint32), "tile_size": np.asarray(tile_size, np.uint32), "samples": np.uint32(samples),
            "max_bounces": np.uint32(max_bounces), "volume_marches": np.uint32(volume_marches), "frame": np.uint32(frame),
            "time_range": np.asarray(time_range, np.float32), "filter": np.asarray([fk, fr, fp[0], fp[1]], np.float32),
            "world": np.frombuffer(bytes(world_bytes), np.uint8), "target_error": np.float32(progressive.target_error),
            "noise_floor": np.float32(progressive.noise_floor), "min_epochs": np.uint32(progressive.min_epochs),
            "outlier_permille": np.uint32(progressive.outlier_permille), "adaptive": np.uint8(bool(progressive.adaptive)),
            "fma_policy": np.uint32(fma_policy)}


def check_key(saved, wanted):
    """ValueError naming the first field of the checkpoint's key that differs from the render's."""
    for name in KEY_FIELDS:
        a, b = np.asarray(saved[name]), np.asarray(wanted[name])
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            shown = "" if name == "world" else f": the checkpoint has {a.tolist()!r}, the render {b.tolist()!r}"
            raise ValueError(f"the checkpoint was made for another {name}{shown}")


def write_checkpoint(path, key, arrays, epochs_run):
    """One .npz: the key, the state arrays of split_state (the active list is implied by the records) and the epochs run so far."""
    data = {"key_" + k: np.asarray(key[k]) for k in KEY_FIELDS}
    data.update({"state_" + k: np.asarray(arrays[k]) for k in STATE_FIELDS})
    data["epochs_run"] = np.uint32(epochs_run)
    with open(path, "wb") as f:  # np.savez would append .npz to a name without it
        np.savez(f, **data)


def read_checkpoint(path):
    """(key, state arrays, epochs run) of a file write_checkpoint made; ValueError for anything else."""
    try:
        with np.load(path, allow_pickle=False) as z:
            key = {k: z["key_" + k] for k in KEY_FIELDS}
            arrays = {k: z["state_" + k] for k in STATE_FIELDS}
            return key, arrays, int(z["epochs_run"])
    except (KeyError, OSError, ValueError) as e:
        raise ValueError(f"{path} is not a progressive checkpoint: {e}") from e
