"""CPU checks of the guided denoiser: its C-ABI entry points are exported, bound and refuse to run without a device or
with NULL handles, and the float64 reference of the filter (tests/atrous_ref.py) behaves as its definition says."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fspt_amd import _lib as L
from fspt_amd import tracer as T
import atrous_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fspt_features", "fspt_read_features", "fspt_denoise", "fspt_draw_denoised")


def test_symbols_exported_and_bound():
    lib = C.CDLL(L.LIB_PATH)
    for n in NEW:
        assert hasattr(lib, n) and n in L.SIGNATURES, n
    assert C.sizeof(L.DenoiseParams) == 16


def test_python_defaults_are_the_header_defaults():
    text = open(os.path.join(ROOT, "include", "fspt.h")).read()
    got = {k: float(re.search(r"#define FSPT_DENOISE_%s ([0-9.]+)" % k.upper(), text).group(1)) for k in T.DENOISE_DEFAULTS}
    assert got == {k: float(v) for k, v in T.DENOISE_DEFAULTS.items()}
    import inspect
    ref = {k: p.default for k, p in inspect.signature(R.atrous).parameters.items() if k in T.DENOISE_DEFAULTS}
    assert ref == T.DENOISE_DEFAULTS  # the reference's defaults are the library's


def test_null_handles_invalid():
    lib = L.lib()
    buf = np.zeros(64, np.float32)
    cp = L.CameraParams()
    assert lib.fspt_features(None, C.byref(cp), 1, 1) == -1
    assert lib.fspt_read_features(None, L.fptr(buf)) == -1
    assert lib.fspt_denoise(None, None, None) == -1
    assert lib.fspt_draw_denoised(None, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -1


def test_no_device():
    """Without a HIP device every new call fails with FSPT_E_NO_DEVICE before it looks at the target (no target can exist
    without a device: a stand-in handle that is never dereferenced)."""
    lib = L.lib()
    if lib.fspt_device_count() > 0:
        pytest.skip("GPU present")
    fake = C.cast(C.create_string_buffer(4096), C.c_void_p)
    buf = np.zeros(64, np.float32)
    cp = L.CameraParams()
    assert lib.fspt_features(fake, C.byref(cp), 1, 1) == -2
    assert lib.fspt_read_features(fake, L.fptr(buf)) == -2
    assert lib.fspt_denoise(fake, None, None) == -2
    assert lib.fspt_draw_denoised(fake, 1.0, 1.0, buf.ctypes.data_as(C.POINTER(C.c_uint8))) == -2
    assert b"no CPU fallback" in lib.fspt_last_error()


def random_inputs(H=12, W=10, seed=0):
    rng = np.random.default_rng(seed)
    acc = np.ones((H, W, 4), np.float32)
    acc[..., :3] = rng.uniform(0, 2, (H, W, 3))
    f = np.zeros((H, W, 8), np.float32)
    f[..., 0:3] = rng.uniform(0.05, 1, (H, W, 3))
    f[..., 3] = rng.uniform(1, 3, (H, W))
    n = rng.normal(size=(H, W, 3)) * 0.2 + [0, 0, 1]
    f[..., 4:7] = n / np.linalg.norm(n, axis=-1, keepdims=True)
    f[..., 7] = 1
    return acc, f


def test_reference_zero_iterations_is_identity():
    acc, f = random_inputs()
    assert np.array_equal(R.atrous(acc, f, 0), acc.astype(np.float64))


def test_reference_constant_is_fixed_point():
    acc = np.ones((9, 11, 4), np.float32); acc[..., :3] = (0.3, 0.6, 1.5)
    f = np.zeros((9, 11, 8), np.float32); f[..., 0:3] = (0.5, 0.25, 0.8); f[..., 3] = 2.0; f[..., 6] = 1.0; f[..., 7] = 1.0
    for k in (1, 3, 5):
        np.testing.assert_allclose(R.atrous(acc, f, k), acc, rtol=1e-12, atol=0)


def plain_b3_atrous(acc, f, iterations):
    """The unguided filter written independently: per pixel, per tap, normalised over the taps inside the image."""
    H, W = acc.shape[:2]
    a = f[..., 0:3].astype(np.float64)
    u = acc[..., :3].astype(np.float64) / np.maximum(a, 1e-3)
    b = [1 / 16, 1 / 4, 3 / 8, 1 / 4, 1 / 16]
    for k in range(iterations):
        s = 1 << k
        v = np.zeros_like(u)
        for y in range(H):
            for x in range(W):
                tot, wsum = np.zeros(3), 0.0
                for j in range(5):
                    for i in range(5):
                        yy, xx = y + (j - 2) * s, x + (i - 2) * s
                        if 0 <= yy < H and 0 <= xx < W:
                            tot += b[i] * b[j] * u[yy, xx]
                            wsum += b[i] * b[j]
                v[y, x] = tot / wsum
        u = v
    return a * u


def test_reference_unguided_is_plain_b3():
    acc, f = random_inputs(seed=3)
    f[2:5, 4:8, 7] = 0  # misses and hit / miss edges: the unguided setting ignores them too
    for k in (1, 2, 3):
        got = R.atrous(acc, f, k, sigma_color=np.inf, sigma_normal=0.0, sigma_depth=np.inf)
        np.testing.assert_allclose(got[..., :3], plain_b3_atrous(acc, f, k), rtol=1e-12, atol=1e-14)
        assert (got[..., 3] == 1).all()


@pytest.mark.parametrize("sigma_normal", [1.0, 128.0])
def test_reference_never_crosses_hit_miss_boundary(sigma_normal):
    acc, f = random_inputs(H=16, W=16, seed=4)
    f[:, 8:, 4:7] = 0; f[:, 8:, 7] = 0; f[:, 8:, 0:3] = 1; f[:, 8:, 3] = 1e5  # right half: misses
    base = R.atrous(acc, f, 4, sigma_color=np.inf, sigma_normal=sigma_normal, sigma_depth=np.inf)
    other = acc.copy(); other[:, 8:, :3] *= 7.0
    moved = R.atrous(other, f, 4, sigma_color=np.inf, sigma_normal=sigma_normal, sigma_depth=np.inf)
    assert np.array_equal(base[:, :8], moved[:, :8])  # the hit side never sees the miss side ...
    assert not np.array_equal(base[:, 8:], moved[:, 8:])  # ... which did change
    other = acc.copy(); other[:, :8, :3] *= 7.0
    moved = R.atrous(other, f, 4, sigma_color=np.inf, sigma_normal=sigma_normal, sigma_depth=np.inf)
    assert np.array_equal(base[:, 8:], moved[:, 8:])  # and the other way round
