"""The random film shared by tests/test_denoise_device.py and tests/test_denoise_variance_device.py.
TEST INFRASTRUCTURE: nothing under rayn_amd/ imports this."""
import numpy as np


def random_film(w, h, seed):
    rng = np.random.default_rng(seed)
    n = w * h
    color = rng.gamma(0.6, 0.5, (n, 3)).astype(np.float32)
    normal = rng.normal(size=(n, 3)).astype(np.float32)
    normal /= np.maximum(np.linalg.norm(normal, axis=1, keepdims=True), 1e-6)
    alpha = rng.choice(np.array([0.0, 0.25, 1.0, 1.0, 1.0], np.float32), n)
    normal[alpha == 0] = 0.0  # background pixels carry no normal, as the film has them
    return {"color": color, "alpha": alpha, "normal": normal}
