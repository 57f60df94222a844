"""numpy restatement of the camera models (include/fspt.h fspt_target_set_camera_model), written from the text of DESIGN 8.15
step by step, not from the kernel.

Two arithmetics.  F32: float32 under DESIGN 2's contract - every product, sum and quotient of float32 arrays is rounded once
(numpy does not contract), `fma` is exposure_ref.fma32, sin / cos / sqrt / division and rnd() come from oracle.math_eval.  F64:
plain float64 numpy, for checking the GEOMETRY of the rule against closed forms (tests/test_camera_model_cpu.py).

rays(...) returns (pos, dir) as [H, W, 4] arrays, row 0 = the bottom row, w = 1 - what fspt_read_rays returns.
"""
import numpy as np

import sobol_ref as SR
from exposure_ref import fma32

MODELS = {"ortho": 1, "fisheye": 2, "equirect": 3, "stereo": 4}


class F32:
    dtype = np.float32
    pi = np.float32(3.14159265)

    @staticmethod
    def _m(op, a, b=None):
        import oracle as O
        a = np.ascontiguousarray(a, np.float32)
        if b is not None:
            a, b = np.broadcast_arrays(a, np.asarray(b, np.float32))
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
        return O.math_eval(op, a.reshape(-1), None if b is None else b.reshape(-1)).reshape(a.shape)

    fma = staticmethod(lambda a, b, c: fma32(a, b, c))
    sin = classmethod(lambda k, x: k._m(0, x))
    cos = classmethod(lambda k, x: k._m(1, x))
    div = classmethod(lambda k, a, b: k._m(5, a, b))
    sqrt = classmethod(lambda k, x: k._m(6, x))
    rnd = classmethod(lambda k, seed: k._m(7, seed))


class F64:
    dtype = np.float64
    pi = np.float64(np.pi)
    fma = staticmethod(lambda a, b, c: a * b + c)
    sin = staticmethod(np.sin)
    cos = staticmethod(np.cos)
    div = staticmethod(lambda a, b: a / b)
    sqrt = staticmethod(np.sqrt)


def _dot(A, a, b):  # fspt_math.hpp: fma(a.z, b.z, fma(a.y, b.y, a.x * b.x))
    return A.fma(a[2], b[2], A.fma(a[1], b[1], a[0] * b[0]))


def _cross(A, a, b):
    return [A.fma(a[1], b[2], -(a[2] * b[1])), A.fma(a[2], b[0], -(a[0] * b[2])), A.fma(a[0], b[1], -(a[1] * b[0]))]


def _normalize(A, a):
    inv = A.div(np.ones_like(a[0]), A.sqrt(_dot(A, a, a)))
    return [a[0] * inv, a[1] * inv, a[2] * inv]


def draws(W, H, rand_base, sampler="reference", seed=0, tick=0):
    """Step 2 in float32: the four draws of every pixel, [4][H, W]."""
    f = np.float32
    x = np.broadcast_to(np.arange(W, dtype=np.uint32)[None, :], (H, W))
    y = np.broadcast_to(np.arange(H, dtype=np.uint32)[:, None], (H, W))
    if sampler == "sobol":
        pix = (y * np.uint32(W) + x).astype(np.uint32)
        return [SR.value(seed, pix, tick, d).astype(f) for d in range(4)]
    fx, fy = x.astype(f) + f(0.5), y.astype(f) + f(0.5)
    s = (fma32(fx, f(H), f(rand_base)) + fy).astype(f)
    out = []
    for _ in range(4):  # rnd(): the value of the seed as it stands (math_eval 7 adds the step itself), then the seed moves on
        out.append(F32.rnd(s))
        s = (s + f(0.211324865405187)).astype(f)
    return out


def rays(model, W, H, P, I, fov_scale, lens, rand_base=0.0, angle=None, ipd=None, sampler="reference", seed=0, tick=0, A=F32, u=None):
    """The rule of DESIGN 8.15 for every pixel of a W x H target.  `u`: the four draws (scalars or [H, W] arrays) instead of
    the sampler's - the geometry tests pass zeros."""
    if isinstance(model, str):
        model = MODELS[model]
    t = A.dtype
    angle = t(np.float32(np.pi if angle is None else angle))
    ipd = t(np.float32(0.064 if ipd is None else ipd))
    two, one, half = t(2.0), t(1.0), t(0.5)
    xi = np.broadcast_to(np.arange(W)[None, :], (H, W))
    yi = np.broadcast_to(np.arange(H)[:, None], (H, W))
    # 1
    fx, fy = xi.astype(t) + half, yi.astype(t) + half
    resx, resy = t(W), t(H)
    # 2
    if u is None:
        u = draws(W, H, rand_base, sampler, seed, tick)
    u0, u1, u2, u3 = (np.broadcast_to(np.asarray(v, np.float32).astype(t), (H, W)) for v in u)
    # 3
    sc = lambda c: np.full((1, 1), np.float32(c)).astype(t)  # (a scalar as a [1, 1] array: every helper sees arrays)
    Iv = [sc(c) for c in I]
    Pv = [sc(c) for c in P]
    fov = sc(fov_scale)
    l0, l1 = t(np.float32(lens[0])), t(np.float32(lens[1]))
    resx, resy, angle, ipd = sc(W), sc(H), sc(angle), sc(ipd)
    bX = _normalize(A, _cross(A, Iv, [sc(0.0), sc(1.0), sc(0.0)]))
    bY = _normalize(A, _cross(A, bX, Iv))
    F = _normalize(A, Iv)
    aspect = A.div(resx, resy)
    # 4
    theta = (u0 * A.pi) * two
    r = A.sqrt(u1) * t(np.float32(0.707))
    px = A.fma(r, A.cos(theta), fx)
    py = A.fma(r, A.sin(theta), fy)
    uu = A.fma(A.div(px, resx), two, -one)
    upper = None
    if model == 4:
        if H % 2:
            raise ValueError("stereo needs an even height")
        upper = yi >= H // 2
        y_half = np.where(upper, t(H // 2), t(0.0)).astype(t)
        vv = A.fma(A.div(py - y_half, resy * half), two, -one)
    else:
        vv = A.fma(A.div(py, resy), two, -one)
    # 5
    full = lambda c: np.broadcast_to(np.asarray(c, t), (H, W)).astype(t)
    o0 = [full(c) for c in Pv]
    d0 = [full(c) for c in F]
    if model == 1:
        a = uu * aspect
        o0 = [A.fma(vv * bY[c], fov, (a * bX[c]) * fov) + Pv[c] for c in range(3)]
    elif model == 2:
        sx, sy = uu * aspect, vv
        rho = A.sqrt(A.fma(sy, sy, sx * sx))
        phi = np.minimum(rho * (angle * half), A.pi)
        sp, cp = A.sin(phi), A.cos(phi)
        with np.errstate(invalid="ignore", divide="ignore"):
            ex, ey = A.div(sx, rho), A.div(sy, rho)
            d = [A.fma(sp, A.fma(ey, bY[c], ex * bX[c]), cp * F[c]) for c in range(3)]
        d0 = [np.where(rho == 0, d0[c], d[c]).astype(t) for c in range(3)]
    elif model in (3, 4):
        lon, lat = uu * A.pi, vv * (A.pi * half)
        sl, cl, sa, ca = A.sin(lon), A.cos(lon), A.sin(lat), A.cos(lat)
        d0 = [A.fma(sa, bY[c], ca * A.fma(sl, bX[c], cl * F[c])) for c in range(3)]
        if model == 4:
            e = np.where(upper, -(ipd * half), ipd * half).astype(t)  # s (ipd / 2): s = -1 for the upper half, the left eye
            o0 = [A.fma(e, A.fma(-sl, F[c], cl * bX[c]), Pv[c]) for c in range(3)]
    else:
        raise ValueError(f"model {model}")
    # 6
    if l1 == 0 or l0 >= 1:
        o, d = o0, d0
    else:
        f = A.div(sc(1.0), sc(1.0) - sc(lens[0]))
        t2 = (u2 * A.pi) * two
        s2, c2 = A.sin(t2), A.cos(t2)
        sq = A.sqrt(u3)
        dof = [(A.fma(s2, bY[c], c2 * bX[c]) * l1) * sq for c in range(3)]
        o = [o0[c] + dof[c] for c in range(3)]
        tgt = [A.fma(f, d0[c], o0[c]) for c in range(3)]
        d = _normalize(A, [tgt[c] - o[c] for c in range(3)])
    # 7
    pos = np.ones((H, W, 4), t)
    dr = np.ones((H, W, 4), t)
    for c in range(3):
        pos[..., c] = o[c]
        dr[..., c] = d[c]
    return pos, dr
