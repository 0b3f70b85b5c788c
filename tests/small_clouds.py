"""Generated clouds that bend the engine's path, shared by tests/test_engine_gpu.py and tests/test_lockstep_gpu.py (numpy only)."""
import numpy as np

DEGENERATE = [(500, 20.0), (50, 5.0), (5, 1.0), (1, 1.0), (4000, 200.0)]  # (points, half extent in x and y [m])


def degenerate_pair(n, scale):
    """Tiny, single-point and extremely sparse clouds (n = 4000 at 200 m: every point its own voxel at all levels): n and
    max(n - 3, 1) points, uniform in a box of +-scale x +-scale x +-2 m."""
    rng = np.random.default_rng(n)
    a = (rng.uniform(-1, 1, (n, 3)) * np.array([scale, scale, 2.0])).astype(np.float32)
    b = (rng.uniform(-1, 1, (max(n - 3, 1), 3)) * np.array([scale, scale, 2.0])).astype(np.float32)
    return a, b


def overflow_box_pair():
    """6 000 and 5 500 points in a 6 x 6 x 4 m box: 300-500 points inside a level-0 search radius, more than the first pass's
    256-key buffer (the engine's deferred large-buffer pass)."""
    rng = np.random.default_rng(5)
    box = np.array([3.0, 3.0, 2.0])
    a = (rng.uniform(-1, 1, (6000, 3)) * box).astype(np.float32)
    b = (rng.uniform(-1, 1, (5500, 3)) * box).astype(np.float32)
    return a, b
