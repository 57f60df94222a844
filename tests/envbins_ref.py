"""env_sampler.js's ProcessEnvRadiance (as fspt_env_bins, scene_build.cpp, states it) restated in Python: per-texel radiance in
numpy float64, box sums by math.fsum - correctly rounded, so independent of the order - and the same recursion.  What
fspt_env_bins_gpu is held against besides the CPU builder itself, and where the tests' maps get their decision margin.

The JS quirk is kept as it is: getRadiance(x, y) reads the four bytes at y * (w * 4) + x * 4 + i.  For integer x, y that is a
texel; for the halves and quarters the halving of odd boxes makes, the index is mostly no integer (`undefined`, NaN) and now
and then one - then it reads four bytes that straddle texels, or a texel of another row.
"""
import math

import numpy as np

W_RGB = (0.2126, 0.7152, 0.0722)


def radiance(env, w, h):
    """(h, w) float64: getRadiance of every texel, in radiance_at's order of operations"""
    e = np.asarray(env, np.uint8).reshape(h, w, 4).astype(np.float64)
    power = np.ldexp(1.0, (e[..., 3] - 128).astype(np.int64))
    n = [power * e[..., i] / 255.0 for i in range(3)]
    return W_RGB[0] * n[0] + W_RGB[1] * n[1] + W_RGB[2] * n[2]


def _radiance_at(data, w, h, x, y):
    base = (y * (w * 4.0)) + (x * 4.0)
    if base != math.floor(base) or not (0 <= base and base + 3 < w * h * 4.0):
        return math.nan
    c = [float(v) for v in data[int(base):int(base) + 4]]
    power = math.ldexp(1.0, int(c[3]) - 128)
    n = [power * c[i] / 255.0 for i in range(3)]
    return W_RGB[0] * n[0] + W_RGB[1] * n[1] + W_RGB[2] * n[2]


def _first_half(data, rad, w, h, x0, y0, xs, ys):
    if not (x0 < xs and y0 < ys):
        return 0.0
    if x0 == math.floor(x0) and y0 == math.floor(y0):
        return math.fsum(rad[int(y0):int(math.ceil(ys)), int(x0):int(math.ceil(xs))].ravel())
    # Off the texel grid the terms are not the map's radiance (2^(a colour byte - 128) can be 2^127) and the parent's
    # `radiance - sub` may cancel without bound: no summation order is as good as another here, so this one path adds in
    # the reference's own order, x outer, y inner.
    sub = 0.0
    x = x0
    while x < xs:
        y = y0
        while y < ys:
            sub += _radiance_at(data, w, h, x, y)
            if sub != sub:
                return math.nan
            y += 1
        x += 1
    return sub


def _to_uint16(v):
    return int(math.trunc(v)) % 65536 if math.isfinite(v) else 0


def _run(env, w, h):
    data = np.asarray(env, np.uint8).reshape(-1)
    rad = radiance(data, w, h)
    total = math.fsum(rad.ravel())
    brightest = float(rad.max())
    min_radiance = max(total / 64, brightest / 2)
    boxes, margins = [], []

    def bisplit(radiance_, x0, y0, x1, y1, depth):
        # (a box of area < 2 or depth > 64 stops whatever its radiance: no decision hangs on the sum)
        if math.isfinite(radiance_) and min_radiance > 0 and (y1 - y0) * (x1 - x0) >= 2 and depth <= 64:
            margins.append(abs(radiance_ - min_radiance) / min_radiance)
        if radiance_ <= min_radiance or (y1 - y0) * (x1 - x0) < 2 or depth > 64:
            boxes.extend((x0, y0, x1, y1))
            return
        vert = (x1 - x0) > (y1 - y0)
        xs, ys = x1, (y1 - y0) / 2 + y0
        if vert:
            xs, ys = (x1 - x0) / 2 + x0, y1
        sub = _first_half(data, rad, w, h, x0, y0, xs, ys)
        bisplit(sub, x0, y0, xs, ys, depth + 1)
        if vert:
            bisplit(radiance_ - sub, xs, y0, x1, y1, depth + 1)
        else:
            bisplit(radiance_ - sub, x0, ys, x1, y1, depth + 1)

    bisplit(total, 0.0, 0.0, float(w), float(h), 0)
    return np.array([_to_uint16(v) for v in boxes], np.uint32), margins, np.array(boxes, np.float64).reshape(-1, 4)


def env_bins(env, w, h):
    """the bins, uint32 [4 n], in the recursion's depth-first order"""
    return _run(env, w, h)[0]


def decision_margin(env, w, h):
    """the smallest |radiance - min_radiance| / min_radiance over every finite stop decision taken (inf when the map is
    black: min_radiance is 0 and every comparison is 0 <= 0, which no summation order changes)"""
    m = _run(env, w, h)[1]
    return min(m) if m else math.inf


def leaves(env, w, h):
    """the leaves' corners as the recursion holds them, float64 [n, 4]: fractional where an odd box was halved"""
    return _run(env, w, h)[2]


def box_sum(rad, box):
    x0, y0, x1, y1 = (int(v) for v in box)
    return math.fsum(rad[y0:y1, x0:x1].ravel())
