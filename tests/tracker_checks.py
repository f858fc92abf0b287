"""What the float trackers' GPU tests share (test_{sgt,b1i,e1t,e1alt,l3}_gpu.py)."""
import numpy as np

_cache = {}


def close(a, b, rtol=1e-6, atol=1e-6):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b) <= rtol * np.abs(b) + atol


def noise(gc, n, fs, file_type=2, seed=21):
    """A seeded record of n samples without a signal (real for file_type 1), made once."""
    key = (n, fs, file_type, seed)
    if key not in _cache:
        _cache[key] = gc.ifgen(n, [], fs=fs, iq=file_type == 2, seed=seed)
    return _cache[key]
