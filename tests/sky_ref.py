"""The sky model of DESIGN 8.17 (include/fspt_tuning.h) restated in numpy, in float64 or float32, and the RGBE encode in exact
float32 steps.  What k_sky_generate is compared with.

Two forms of the same model:
  sky(...)       the order of operations the kernel uses.  A point on a ray is never formed: with a = |p|^2 - Re^2 one has
                 |o + t d|^2 - Re^2 = (|o|^2 - Re^2) + t (2 o.d + t), the height (|p| - Re) = a / (|p| + Re), and the far hit of
                 a ray from p along s with the sphere R at -p.s + sqrt((p.s)^2 - (|p|^2 - R^2)).  In float32 that keeps a height's
                 error at 1e-7 of the height instead of half a metre (|p| = 6.36e6 m has an ulp of 0.5 m).
  sky_text(...)  the model as its text states it, with points and norms, float64 only.  test_sky_cpu.py holds the two together.
"""
import math

import numpy as np

RE, RA, HR, HM, G = 6360000.0, 6420000.0, 7994.0, 1200.0, 0.76
BETA_R = (5.8e-6, 13.5e-6, 33.1e-6)
DEFAULTS = dict(turbidity=1.0, sun_intensity=20.0, sun_radius=0.02, gain=1.0, ground_albedo=(0.3, 0.3, 0.3),
                view_samples=16, light_samples=8)


def params(**kw):
    p = dict(DEFAULTS, **kw)
    alb = np.atleast_1d(np.asarray(p["ground_albedo"], np.float64))
    p["ground_albedo"] = tuple(np.repeat(alb, 3)[:3]) if alb.size == 1 else tuple(alb)
    return p


def unit_sun(sun_dir):
    """the library's normalisation: float32 components, the length in float64, the quotient rounded to float32"""
    s = np.asarray(sun_dir, np.float32).astype(np.float64)
    return (s / math.sqrt(float((s * s).sum()))).astype(np.float32)


def directions(w, h, dtype):
    """d, (h, w) each component: the inverse of envSample at envTheta = 0, texel centres, row 0 = up"""
    f = dtype
    u = (np.arange(w, dtype=f) + f(0.5)) / f(w)
    v = (np.arange(h, dtype=f) + f(0.5)) / f(h)
    pi = f(np.float32(math.pi)) if dtype is np.float32 else f(math.pi)
    theta, phi = f(2.0) * pi * u, pi * v
    sp, cp = np.sin(phi)[:, None], np.cos(phi)[:, None]
    dx = np.cos(theta)[None, :] * sp
    dz = np.sin(theta)[None, :] * sp
    dy = np.broadcast_to(cp, dx.shape).copy()
    return dx, dy, dz


def _consts(dtype):
    f = dtype
    # |o|^2 - Re^2 = (oy - Re)(oy + Re) = 12 720 001, |o|^2 - Ra^2 = (oy - Ra)(oy + Ra), Ra^2 - Re^2 = (Ra - Re)(Ra + Re):
    # every factor is an integer below 2^24, so only the products round in float32
    return dict(re=f(RE), hr=f(HR), hm=f(HM), oy=f(RE + 1.0), ce=f(2 * RE + 1.0), ca=f(RE + 1.0 - RA) * f(RE + 1.0 + RA),
                k=f(RA - RE) * f(RA + RE), re2=f(RE) * f(RE))


def _height(a, K):
    return a / (np.sqrt(K["re2"] + a) + K["re"])


def _light_ray(a, ps, M, K, f):
    """optical depths of the light ray from points with |p|^2 - Re^2 = a, p.s = ps; lit = no midpoint below the ground"""
    tl = -ps + np.sqrt(ps * ps - (a - K["k"]))
    dl = tl / f(M)
    lit = np.ones(a.shape, bool)
    lR = np.zeros(a.shape, f)
    lM = np.zeros(a.shape, f)
    for j in range(M):
        l = (f(j) + f(0.5)) * dl
        hl = _height(a + l * (f(2.0) * ps + l), K)
        lit &= ~(hl < 0)
        lR = lR + np.exp(-hl / K["hr"]) * dl
        lM = lM + np.exp(-hl / K["hm"]) * dl
    return lit, lR, lM


def sky(sun_dir, w, h, dtype=np.float64, **kw):
    """Linear radiance (h, w, 3) in `dtype`, in the kernel's order of operations.  Also returns a dict with `mu`, `ground`
    and `disc` (the texels of the sun's disc) for the tests."""
    p = params(**kw)
    f = dtype
    K = _consts(f)
    s = unit_sun(sun_dir).astype(f)
    N, M = int(p["view_samples"]), int(p["light_samples"])
    turb, I, rad, gain = (float(np.float32(p[k])) for k in ("turbidity", "sun_intensity", "sun_radius", "gain"))
    bR = [f(np.float32(b)) for b in BETA_R]
    bM, bMe = f(turb * 21e-6), f(1.1 * turb * 21e-6)
    alb_pi = [f(float(np.float32(a)) / math.pi) for a in p["ground_albedo"]]
    cos_r, disc_scale = f(math.cos(rad)), f(I / (math.pi * rad * rad))
    I, gain = f(I), f(gain)
    pi = f(np.float32(math.pi)) if f is np.float32 else f(math.pi)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        dx, dy, dz = directions(w, h, f)
        mu = (dx * s[0] + dy * s[1]) + dz * s[2]
        b = K["oy"] * dy
        t_atm = -b + np.sqrt(b * b - K["ca"])
        disc_e = b * b - K["ce"]
        t_gnd = np.where(disc_e >= 0, -b - np.sqrt(np.maximum(disc_e, 0)), f(-1.0)).astype(f)
        ground = t_gnd > 0
        t_max = np.where(ground, t_gnd, t_atm).astype(f)
        ds = t_max / f(N)
        os_ = K["oy"] * s[1]
        tR = np.zeros((h, w), f)
        tM = np.zeros((h, w), f)
        sumR = [np.zeros((h, w), f) for _ in range(3)]
        sumM = [np.zeros((h, w), f) for _ in range(3)]
        for i in range(N):
            t = (f(i) + f(0.5)) * ds
            a = K["ce"] + t * (f(2.0) * b + t)
            hv = _height(a, K)
            rR = np.exp(-hv / K["hr"]) * ds
            rM = np.exp(-hv / K["hm"]) * ds
            tR = tR + rR
            tM = tM + rM
            lit, lR, lM = _light_ray(a, os_ + t * mu, M, K, f)
            for c in range(3):
                T = np.exp(-(bR[c] * (tR + lR) + bMe * (tM + lM)))
                sumR[c] = np.where(lit, sumR[c] + T * rR, sumR[c])
                sumM[c] = np.where(lit, sumM[c] + T * rM, sumM[c])
        g = f(np.float32(G)) if f is np.float32 else f(G)
        m2 = f(1.0) + mu * mu
        pR = f(3.0) / (f(16.0) * pi) * m2
        den = f(1.0) + g * g - f(2.0) * g * mu
        pM = f(3.0) / (f(8.0) * pi) * ((f(1.0) - g * g) * m2) / ((f(2.0) + g * g) * (den * np.sqrt(den)))
        ag = K["ce"] + t_gnd * (f(2.0) * b + t_gnd)
        psg = os_ + t_gnd * mu
        ns = psg / np.sqrt(K["re2"] + ag)
        glit, glR, glM = _light_ray(np.where(ground, ag, f(0.0)).astype(f), np.where(ground, psg, f(0.0)).astype(f), M, K, f)
        disc = ~ground & (mu >= cos_r)
        out = np.zeros((h, w, 3), f)
        for c in range(3):
            L = I * (sumR[c] * bR[c] * pR + sumM[c] * bM * pM)
            Tv = np.exp(-(bR[c] * tR + bMe * tM))
            E = Tv * alb_pi[c] * (I * np.exp(-(bR[c] * glR + bMe * glM)) * ns)
            L = np.where(ground & glit & (ns > 0), L + E, L)
            L = np.where(disc, L + disc_scale * Tv, L)
            out[..., c] = L * gain
    return out.astype(f), dict(mu=mu, ground=ground, disc=disc)


def sky_text(sun_dir, w, h, **kw):
    """The model as the text of DESIGN 8.17 states it, with points and norms, float64."""
    p = params(**kw)
    s = unit_sun(sun_dir).astype(np.float64)
    N, M = int(p["view_samples"]), int(p["light_samples"])
    turb, I, rad, gain = (float(np.float32(p[k])) for k in ("turbidity", "sun_intensity", "sun_radius", "gain"))
    bR = np.array([float(np.float32(b)) for b in BETA_R])
    bM = turb * 21e-6
    alb = np.array([float(np.float32(a)) for a in p["ground_albedo"]])
    dx, dy, dz = directions(w, h, np.float64)
    out = np.zeros((h, w, 3))
    o = np.array([0.0, RE + 1.0, 0.0])

    def hit(org, d, R, far):
        b = float(org @ d)
        c = float(org @ org) - R * R
        disc = b * b - c
        if disc < 0:
            return None
        q = math.sqrt(disc)
        return -b + q if far else -b - q

    def light(pnt):
        tl = hit(pnt, s, RA, True)
        dl = tl / M
        lR = lM = 0.0
        for j in range(M):
            q = pnt + s * ((j + 0.5) * dl)
            hq = math.sqrt(float(q @ q)) - RE
            if hq < 0:
                return None
            lR += math.exp(-hq / HR) * dl
            lM += math.exp(-hq / HM) * dl
        return lR, lM

    for y in range(h):
        for x in range(w):
            d = np.array([dx[y, x], dy[y, x], dz[y, x]])
            mu = float(d @ s)
            t_atm = hit(o, d, RA, True)
            t_gnd = hit(o, d, RE, False)
            ground = t_gnd is not None and t_gnd > 0
            t_max = t_gnd if ground else t_atm
            ds = t_max / N
            tR = tM = 0.0
            sumR = np.zeros(3)
            sumM = np.zeros(3)
            for i in range(N):
                pnt = o + d * ((i + 0.5) * ds)
                hi = math.sqrt(float(pnt @ pnt)) - RE
                rR, rM = math.exp(-hi / HR) * ds, math.exp(-hi / HM) * ds
                tR += rR
                tM += rM
                lr = light(pnt)
                if lr is None:
                    continue
                T = np.exp(-(bR * (tR + lr[0]) + 1.1 * bM * (tM + lr[1])))
                sumR += T * rR
                sumM += T * rM
            pR = 3.0 / (16.0 * math.pi) * (1 + mu * mu)
            pM = 3.0 / (8.0 * math.pi) * (1 - G * G) * (1 + mu * mu) / ((2 + G * G) * (1 + G * G - 2 * G * mu) ** 1.5)
            L = I * (sumR * bR * pR + sumM * bM * pM)
            Tv = np.exp(-(bR * tR + 1.1 * bM * tM))
            if ground:
                pg = o + d * t_gnd
                n = pg / math.sqrt(float(pg @ pg))
                ns = float(n @ s)
                lr = light(pg)
                if ns > 0 and lr is not None:
                    L = L + Tv * alb / math.pi * (I * np.exp(-(bR * lr[0] + 1.1 * bM * lr[1])) * ns)
            elif mu >= math.cos(rad):
                L = L + I * Tv / (math.pi * rad * rad)
            out[y, x] = L * gain
    return out


def encode(lin):
    """RGBE bytes (h, w, 4) of float32 radiance (h, w, 3): non-finite or negative -> 0; e = the smallest integer with 2^e >=
    max(r, g, b, 1e-6), from the float's exponent and mantissa fields, clamped to [-127, 127]; bytes floor(c 2^-e 255 + 0.5)
    clamped to [0, 255], every step in float32; E = e + 128."""
    c = np.asarray(lin, np.float32).copy()
    c[~(np.isfinite(c) & (c > 0))] = np.float32(0)
    m = np.maximum(c.max(-1), np.float32(1e-6)).astype(np.float32)
    bits = m.view(np.uint32)
    e = ((bits >> 23) & 255).astype(np.int32) - 127 + ((bits & 0x7FFFFF) != 0)
    e = np.clip(e, -127, 127).astype(np.int32)
    q = np.ldexp(c, -e[..., None]).astype(np.float32)  # exact (or a correctly rounded subnormal)
    q = np.floor(q * np.float32(255.0) + np.float32(0.5)).astype(np.float32)
    q = np.clip(q, np.float32(0), np.float32(255))
    return np.concatenate([q.astype(np.uint8), (e + 128).astype(np.uint8)[..., None]], -1)


def rel_error(got, ref, intensity=20.0, gain=1.0):
    """the largest |got - ref| / (|ref| + 1e-6 I gain) over texels and channels, in float64"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return float((np.abs(got - ref) / (np.abs(ref) + 1e-6 * intensity * gain)).max())
