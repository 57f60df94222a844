"""The maps and sun positions tests/test_sky_cpu.py and tests/test_sky_gpu.py share.  test_sky_cpu.py checks the
conditions the GPU tests rest on - every map's decision margin, every generator case's distance from the disc's edge - with
the float64 restatements alone."""
import math

import numpy as np

import sky_ref as K

GEN_SIZES = ((2, 1), (8, 4), (64, 32), (65, 33), (127, 3))
GEN_SAMPLES = ((1, 1), (16, 8))
GEN_TURBIDITY = (0.0, 8.0)


def texel_centre(w, h, x, y):
    dx, dy, dz = K.directions(w, h, np.float64)
    return (float(dx[y, x]), float(dy[y, x]), float(dz[y, x]))


def suns(w, h):
    """name -> direction: the zenith, 30 degrees up, on the horizon, 10 degrees below it, and exactly on a texel's centre"""
    el = lambda deg, az=0.7: (math.cos(az) * math.cos(math.radians(deg)), math.sin(math.radians(deg)), math.sin(az) * math.cos(math.radians(deg)))
    return {"zenith": (0.0, 1.0, 0.0), "up30": el(30.0), "horizon": el(0.0), "below10": el(-10.0),
            "centre": texel_centre(w, h, (2 * w) // 3, h // 4)}


def generator_cases(w, h, samples):
    for turb in GEN_TURBIDITY:
        for name, sun in suns(w, h).items():
            yield f"{name}-t{turb:g}", sun, dict(turbidity=turb, view_samples=samples[0], light_samples=samples[1])


def synthetic(w, h):
    from fspt_amd import scene as S
    return np.asarray(S.synthetic_env(w, h)[0], np.uint8)


def ref_sky_rgbe(w, h, sun=(0.5, 0.6, 0.4), **kw):
    """a generated sky's bytes from the float32 restatement: a map `with a sun` that needs no device"""
    lin, _ = K.sky(sun, w, h, dtype=np.float32, **kw)
    return K.encode(lin).reshape(-1)


def hot_texel(w, h, x, y):
    env = np.zeros((h, w, 4), np.uint8)
    env[y, x] = (200, 180, 90, 131)
    return env.reshape(-1)


BOX_SIZES = ((1, 1), (63, 2), (64, 64), (65, 3), (129, 65), (256, 128))
BINS_SYNTHETIC = ((1, 1), (2, 1), (8, 4), (64, 32), (256, 128))
BINS_NAN = ((7, 3), (15, 7), (33, 17))


def box_map(w, h):
    return ref_sky_rgbe(w, h, view_samples=4, light_samples=2)


def boxes_for(w, h):
    """the whole map, single texels, single rows and columns, and boxes that straddle every multiple of 64"""
    b = [(0, 0, w, h), (0, 0, 1, 1), (w - 1, h - 1, w, h), (w // 2, h // 2, w // 2 + 1, h // 2 + 1), (0, 0, 0, 0), (w, h, w, h)]
    b += [(0, y, w, y + 1) for y in sorted({0, h // 2, h - 1})]
    b += [(x, 0, x + 1, h) for x in sorted({0, w // 2, w - 1})]
    for m in range(64, w, 64):
        b += [(m - 1, 0, m + 1, h), (m, 0, w, h), (0, 0, m, h), (m - 1, h // 3, min(m + 2, w), h // 3 + 1)]
    for m in range(64, h, 64):
        b += [(0, m - 1, w, m + 1), (0, m, w, h), (0, 0, w, m), (w // 3, m - 1, w // 3 + 1, min(m + 2, h))]
    return np.array(b, np.uint32)


def bins_maps():
    """name -> (env, w, h): every map fspt_env_bins_gpu is held against fspt_env_bins on"""
    import os
    out = {}
    for w, h in BINS_SYNTHETIC:
        out[f"synthetic_{w}x{h}"] = (synthetic(w, h), w, h)
        out[f"sky_{w}x{h}"] = (ref_sky_rgbe(w, h, view_samples=4, light_samples=2), w, h)
    out["zero_16x8"] = (np.zeros(16 * 8 * 4, np.uint8), 16, 8)
    out["hot_32x16"] = (hot_texel(32, 16, 21, 5), 32, 16)
    for w, h in BINS_NAN:
        out[f"odd_{w}x{h}"] = (synthetic(w, h), w, h)
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "js_env_bins_odd.npz"))
    out["golden_odd"] = (np.asarray(g["env"], np.uint8), int(g["env_w"]), int(g["env_h"]))
    return out
