"""The random HDR film shared by tests/test_display.py (CPU) and tests/test_display_device.py (GPU).
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np

ADVERSARIAL = [np.nan, np.inf, -np.inf, -1.0, -0.0, 0.0, 3e38, -3e38, 1.0, 1e-4]


def film(width, height, seed, adversarial=True, with_background=True, with_alpha=True):
    """A random HDR film in film order: colour (n, 3) log-uniform over about six decades, a dim background, an alpha in [0, 1]; with
    `adversarial`, every tenth component or so is one of ADVERSARIAL."""
    rng = np.random.default_rng(seed)
    n = width * height
    color = np.exp(rng.uniform(-8.0, 6.0, (n, 3))).astype(np.float32)
    background = rng.uniform(0.0, 0.5, (n, 3)).astype(np.float32) if with_background else None
    alpha = rng.uniform(0.0, 1.0, n).astype(np.float32) if with_alpha else None
    if adversarial:
        for a in (color, background, alpha):
            if a is not None:
                flat = a.reshape(-1)
                idx = rng.choice(flat.size, max(1, flat.size // 10), replace=False)
                flat[idx] = rng.choice(np.array(ADVERSARIAL, np.float32), len(idx))
    return color, background, alpha
