"""CPU checks of the guided denoiser: its C-ABI entry points are exported, bound and refuse to run without a device or
with NULL handles, the float64 reference of the filter (tests/atrous_ref.py) behaves as its definition says, and the
synthetic inputs the GPU sweep runs k_atrous on (tests/atrous_inputs.py) reach every edge and tell each of a list of
deliberately wrong filters from the right one by more than the sweep's tolerance."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from fspt_amd import _lib as L
from fspt_amd import tracer as T
import atrous_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("fspt_features", "fspt_read_features", "fspt_denoise", "fspt_draw_denoised", "fspt_denoise_eval")


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
    prm = L.DenoiseParams(4, 4.0, 32.0, 0.05)
    for args in ((None, L.fptr(buf)), (L.fptr(buf), None)):  # NULL accumulator, NULL features
        assert lib.fspt_denoise_eval(0, *args, 2, 2, C.byref(prm), L.fptr(buf)) == -1
    assert lib.fspt_denoise_eval(0, L.fptr(buf), L.fptr(buf), 2, 2, None, None) == -1  # NULL out
    assert b"fspt_denoise_eval: NULL argument" in lib.fspt_last_error()


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
    # the test hook: the same code as fspt_denoise for the parameters it would refuse on a device (there the device
    # check comes first too), and for the defaults
    for prm in (None, L.DenoiseParams(4, 4.0, 32.0, 0.05), L.DenoiseParams(17, 1, 128, 0.1), L.DenoiseParams(5, 1, np.inf, 0.1)):
        assert lib.fspt_denoise_eval(0, L.fptr(buf), L.fptr(buf), 2, 2, C.byref(prm) if prm else None, L.fptr(buf)) == -2
        assert b"no CPU fallback" in lib.fspt_last_error()
    with pytest.raises(L.FsptError) as e:
        T.denoise_eval(np.zeros((3, 2, 4), np.float32), np.zeros((3, 2, 8), np.float32), iterations=2)
    assert e.value.code == -2


def test_denoise_eval_python_arguments_validated():
    """Shapes and parameter names are checked before the library is called (no device needed to get there)."""
    from fspt_amd import denoise_eval
    acc, f = np.zeros((3, 2, 4), np.float32), np.zeros((3, 2, 8), np.float32)
    for a, b in ((acc[..., :3], f), (acc, f[..., :7]), (acc, f[:2]), (acc[0], f[0])):
        with pytest.raises(ValueError):
            denoise_eval(a, b)
    with pytest.raises(TypeError):
        denoise_eval(acc, f, sigma=1.0)


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


# ---- the synthetic inputs of the GPU sweep (tests/atrous_inputs.py) ----------------------------------------------------
import atrous_inputs as I  # noqa: E402


def excess(got, ref, rtol=1e-4, atol=1e-6):
    """How many times the GPU tests' bound (rtol where |ref| > 1e-3, atol elsewhere) |got - ref| reaches at its
    worst pixel; inf where got is not finite."""
    if not np.isfinite(got).all():
        return np.inf
    big = np.abs(ref) > 1e-3
    rel = (np.abs(got[big] - ref[big]) / np.abs(ref[big])).max(initial=0.0)
    return max(rel / rtol, np.abs(got[~big] - ref[~big]).max(initial=0.0) / atol)


def test_synthetic_inputs_reach_every_edge():
    acc, f = I.synthetic(80, 120)
    acc2, f2 = I.synthetic(80, 120)
    assert np.array_equal(acc, acc2) and np.array_equal(f, f2)  # deterministic
    h, n, z, a = f[..., 7], f[..., 4:7], f[..., 3], f[..., 0:3]
    nlen = np.linalg.norm(n, axis=-1)
    hit, miss = h > 0, h == 0
    assert (miss & (nlen == 0) & (z == 1e5) & (a == 1).all(-1)).sum() > 100  # misses as k_features writes them
    assert (miss & (nlen > 0)).sum() > 50                                   # misses with a normal (the cut on h alone)
    assert ((h > 0) & (h < 1)).sum() > 100                                  # seams with fractional coverage
    assert (hit & (nlen == 0)).sum() > 50                                   # hits with a zero-length normal
    assert (hit & (a == 0).all(-1)).sum() > 50 and (hit & (a == 0).any(-1) & (a > 0).any(-1)).sum() > 50  # black albedo
    assert (hit & (z == 0)).sum() > 50                                      # z = 0 exactly
    assert acc[..., :3].max() > 512 and (acc[..., :3] == 0).all(-1).sum() > 100  # fireflies and exact zeros
    # equal neighbouring normals whose float32 cosine rounds above 1 (what the clamp is for), and smooth-field pairs
    c = I.cosine_f32(n[:, 1:], n[:, :-1])
    both = hit[:, 1:] & hit[:, :-1] & (nlen[:, 1:] > 0) & (nlen[:, :-1] > 0)
    assert ((c > 1) & both).sum() > 100 and ((c < 0.9999) & (c > 0.99) & both).sum() > 100
    # depth discontinuities between neighbouring hits
    assert ((np.abs(z[:, 1:] - z[:, :-1]) > 0.5) & hit[:, 1:] & hit[:, :-1]).sum() > 50


MUTATION_CASES = [(80, 120, {}), (80, 120, dict(sigma_color=np.inf)), (17, 16, dict(iterations=2))]


@pytest.mark.parametrize("mutant", R.MUTANTS)
def test_inputs_detect_each_mutant(mutant):
    """Each deliberate defect of the reference (atrous_ref.MUTANTS) moves some pixel of one of the GPU sweep's inputs by
    more than the sweep's bound: the sweep would catch the same defect in the kernel."""
    worst = []
    for H, W, kw in MUTATION_CASES:
        acc, f = I.synthetic(H, W)
        ref = R.atrous(acc, f, **kw)
        assert np.isfinite(ref).all()
        worst.append(excess(R.atrous(acc, f, **kw, mutant=mutant), ref))
    print(f"{mutant}: largest deviation {max(worst):.3g} x the tolerance; per case {[f'{w:.3g}' for w in worst]}")
    assert max(worst) > 1, (mutant, worst)


def test_reference_finite_at_every_accepted_edge():
    """The reference itself: finite for every parameter edge the GPU sweep uses, the centre tap's weight 1 included when
    sigma_depth is the smallest float32 (its scaled denominator underflows in float32, not here)."""
    acc, f = I.synthetic(17, 16)
    for kw in (dict(sigma_normal=1e9), dict(sigma_depth=float(np.finfo(np.float32).smallest_subnormal)),
               dict(sigma_depth=1e-6), dict(sigma_color=0.0), dict(iterations=16)):
        assert np.isfinite(R.atrous(acc, f, **kw)).all(), kw
