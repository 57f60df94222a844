"""float64 numpy restatement of SVGF variance guidance (include/fspt_tuning.h): the checker the GPU tests
compare k_temporal_blend<true>, k_svgf_variance and k_atrous<true> against.  Layouts are the library's: hist (H, W, 4) =
rgb, history length; moments (H, W, 2) = M1, M2; features (H, W, 8) = albedo.rgb, depth, normal.xyz, coverage.

Operation order (what the identities of tests/test_svgf_cpu.py rely on):

  moments   u = I.rgb / max(a, 1e-3); l = 0.2126 u.r + 0.7152 u.g + 0.0722 u.b; m = (l, l l).  The history of the moments
            is blended by temporal_ref.blend itself - the colour's taps, tests, weights and factor - with (M1, M2, 0, length)
            in the history's place and (l, l l, 0) in the input's: Mout = Hm + (m - Hm) a; no tap or no history: m.
  variance  Fe = hist.w / n.  Fe >= 4: v = max(0, M2 - M1 M1) / Fe.  Else, over q = p + (i, j), i, j in -3..3 inside the
            image, w = wn wz of atrous_ref at step 1 (the centre weighs 1): S1 = sum w M1 / sum w, S2 = sum w M2 / sum w,
            v = max(0, S2 - S1 S1) / max(Fe, 1).
  filter    u0 = hist.rgb / max(a, 1e-3), var0 = v.  Iteration k, step s = 2^k:
            gv_p = sum g var(q) / sum g over q = p + (i, j), i, j in -1..1 inside the image, g = (1,2,1)(1,2,1)/16;
            w = B3[i] B3[j] [q inside], then times wl = exp(-|L(u_p) - L(u_q)| / (sl sqrt(gv_p) + 1e-4)) unless sl = +inf,
            then times wn, then times wz - atrous_ref's order, its wn and wz, sigma_depth scaled by s;
            u'(p) = sum w u(q) / sum w;  var'(p) = sum w w var(q) / (sum w)^2.
            out = (a u_K, 1), the output variance is var_K.  K = 0: out = hist, var_K = v."""
import numpy as np

import atrous_ref as A
import temporal_ref as T

B3 = A.B3
G3 = np.array([1.0, 2.0, 1.0]) / 4.0
MIN_HISTORY = 4.0
WINDOW = 3
DEFAULTS = {"iterations": 4, "sigma_color": 8.0, "sigma_normal": 32.0, "sigma_depth": 0.05}  # include/fspt_tuning.h FSPT_SVGF_*


def demodulate(c, features):
    a = np.asarray(features, np.float64)[..., 0:3]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.asarray(c, np.float64)[..., :3] / np.maximum(a, 1e-3)


def frame_moments(I, features):
    """m = (l, l l) of the demodulated input."""
    l = A.luma(demodulate(I, features))
    return np.stack([l, l * l], -1)


def blend_moments(I, M, G, hist, mom_hist, g_prev, features, n, **params):
    """Mout of the blend pass: temporal_ref.blend's own taps and factor on the moments.  hist / mom_hist None: m."""
    m = frame_moments(I, features)
    if hist is None or mom_hist is None:
        return m
    H, W = m.shape[:2]
    packed_in = np.concatenate([m, np.zeros((H, W, 2))], -1)
    packed_hist = np.concatenate([np.asarray(mom_hist, np.float64), np.zeros((H, W, 1)), np.asarray(hist, np.float64)[..., 3:4]], -1)
    out, _ = T.blend(packed_in, M, G, packed_hist, g_prev, n, **params)
    return out[..., :2]


def edge_weight(features, dy, dx, s, sigma_normal, sigma_depth):
    """(wn, wz, inside) of the tap q = p + (dy, dx) as atrous_ref computes them at step s; wn is 1 at the centre."""
    f = np.asarray(features, np.float64)
    z, n, h = f[..., 3], f[..., 4:7], f[..., 7]
    hit = h != 0
    nlen = np.sqrt((n * n).sum(-1))
    zq, valid = A.tap(z, dy, dx)
    nq, _ = A.tap(n, dy, dx)
    hq, _ = A.tap(hit, dy, dx)
    lq, _ = A.tap(nlen, dy, dx)
    wn = np.ones(z.shape)
    if sigma_normal != 0 and (dy, dx) != (0, 0):
        both_miss = ~hit & ~hq
        cut = (nlen == 0) | (lq == 0) | (hit != hq)
        with np.errstate(invalid="ignore", divide="ignore"):
            cos = np.minimum((n * nq).sum(-1) / (nlen * lq), 1.0)
            wn = np.maximum(0.0, np.where(cut, 0.0, cos)) ** sigma_normal
        wn = np.where(both_miss, 1.0, np.where(cut, 0.0, wn))
    wz = np.ones(z.shape)
    if not np.isinf(sigma_depth):
        zs = sigma_depth * s * np.maximum(z, 1e-3)
        with np.errstate(invalid="ignore", divide="ignore"):
            wz = np.where(z == zq, 1.0, np.exp(-np.abs(z - zq) / zs))
    return wn, wz, valid


def variance(hist, moments, features, n, sigma_normal=32.0, sigma_depth=0.05):
    """(v, scale): the variance estimate and the magnitude its float32 cancellation error is relative to - M2 / Fe on the
    temporal branch, S2 / max(Fe, 1) on the spatial one (v is a difference of two terms of that size)."""
    hist = np.asarray(hist, np.float64); mom = np.asarray(moments, np.float64)
    Fe = hist[..., 3] / float(n)
    M1, M2 = mom[..., 0], mom[..., 1]
    temporal = Fe >= MIN_HISTORY
    s1 = np.zeros(Fe.shape); s2 = np.zeros(Fe.shape); sw = np.zeros(Fe.shape)
    for j in range(-WINDOW, WINDOW + 1):
        for i in range(-WINDOW, WINDOW + 1):
            wn, wz, valid = edge_weight(features, j, i, 1, sigma_normal, sigma_depth)
            w = np.where(valid, 1.0 if (i, j) == (0, 0) else wn * wz, 0.0)
            q1, _ = A.tap(M1, j, i)
            q2, _ = A.tap(M2, j, i)
            s1 += w * q1; s2 += w * q2; sw += w
    S1, S2 = s1 / sw, s2 / sw
    with np.errstate(invalid="ignore", divide="ignore"):
        v = np.where(temporal, np.maximum(0.0, M2 - M1 * M1) / Fe, np.maximum(0.0, S2 - S1 * S1) / np.maximum(Fe, 1.0))
        scale = np.where(temporal, np.maximum(M2, M1 * M1) / Fe, np.maximum(S2, S1 * S1) / np.maximum(Fe, 1.0))
    return v, scale


def blur3(var):
    num = np.zeros(var.shape); den = np.zeros(var.shape)
    for j in (-1, 0, 1):
        for i in (-1, 0, 1):
            q, valid = A.tap(var, j, i)
            g = G3[i + 1] * G3[j + 1] * valid
            num += g * q; den += g
    return num / den


def guided_atrous(hist, var, features, iterations=4, sigma_color=8.0, sigma_normal=32.0, sigma_depth=0.05, cond=None):
    """(out (H, W, 4), var_K (H, W)) of the variance-guided iterations; sigma_color is sigma_l.  cond: a list that receives,
    per iteration, R_k = max_p L(u_p) / lden_p - how many times its own denominator a pixel's luminance is, the factor by
    which a relative error of the luminances grows in wl's exponent."""
    c = np.asarray(hist, np.float64)
    var = np.asarray(var, np.float64).copy()
    if iterations == 0:
        return c.copy(), var
    a = np.asarray(features, np.float64)[..., 0:3]
    u = demodulate(c, features)
    for k in range(iterations):
        s = 2 ** k
        Lp = A.luma(u)
        if not np.isinf(sigma_color):
            lden = sigma_color * np.sqrt(blur3(var)) + 1e-4
            if cond is not None:
                with np.errstate(invalid="ignore"):
                    cond.append(float(np.nanmax(np.abs(Lp) / lden)))
        num = np.zeros_like(u); den = np.zeros(u.shape[:2]); vnum = np.zeros(u.shape[:2])
        for j in range(-2, 3):
            for i in range(-2, 3):
                uq, valid = A.tap(u, j * s, i * s)
                vq, _ = A.tap(var, j * s, i * s)
                wn, wz, _ = edge_weight(features, j * s, i * s, s, sigma_normal, sigma_depth)
                w = B3[i + 2] * B3[j + 2] * valid
                if not np.isinf(sigma_color):
                    with np.errstate(invalid="ignore"):
                        w = w * np.exp(-np.abs(Lp - A.luma(uq)) / lden)
                if sigma_normal != 0 and (i, j) != (0, 0):
                    w = w * wn
                if not np.isinf(sigma_depth):
                    w = w * wz
                with np.errstate(invalid="ignore"):
                    num += w[..., None] * uq
                    vnum += w * w * vq
                den += w
        with np.errstate(invalid="ignore", divide="ignore"):
            u = num / den[..., None]
            var = vnum / (den * den)
    out = np.ones(c.shape)
    out[..., :3] = a * u
    return out, var


U32 = 2.0 ** -24


def guided_atrous_bounded(hist, var, features, iterations=4, sigma_color=8.0, sigma_normal=32.0, sigma_depth=0.05):
    """(out, var_K, E_out (H, W, 3), E_var (H, W)): guided_atrous and, PER PIXEL, a bound on how far a float32 run of the same
    operations can be from it - from this function's own float64 states, never from the run under test.  u = 2^-24.
    Carried per pixel: E (H, W, 3), the absolute error of u, and Av (H, W), that of var.  E_0 = 2 u u0 (the division, and
    float32(1e-3) for 1e-3 in the clamp), Av_0 = 0 (the run is fed the same v).  One iteration at p:
      lden   the blur has exact weights and <= 9 non-negative terms (9 u), a division, a square root, a product and a sum:
             gv' within blur(Av) + 11 u gv of gv, so lden' / lden within e^(+-el), el from sl sqrt(gv +- that) + 1e-4, + 5 u.
      wl     L' is within luma(E) + 3 u L of L (three products, two sums of non-negative terms), the subtraction, the division,
             the 1.4427 and exp2f add 8 u x and 4 u: the exponent x = |Lp - Lq| / lden is off by at most
             dx = ((EL_p + EL_q + 3 u (Lp + Lq)) / lden) e^el + x (expm1(el) + 8 u).
      wn wz  off by factors within e^dw, dw = 20 u sn + 264 u (test_denoise_gpu.sigma_normal_rtol's cosine bound; the depth
             exponent's three roundings below 88); the centre tap is exact (x = 0, no wn, dz = 0).
      w      so |w' - w| <= dW = w expm1(dx + dw + 6 u) + 1e-36 (a float32 weight that underflows is off by itself), and
             never more than max(B3 B3 - w, w): wl, wn and wz are at most 1 on both sides, so 0 <= w' <= B3 B3.
      u      sum w (u_q - out) = 0, hence out' - out = (sum (w' - w)(u_q - out) + sum w' (u'_q - u_q)) / sum w' + rounding:
             E' = (sum dW |u_q - out| + sum (w + dW) E_q + 27 u sum (w + dW)(|u_q| + E_q)) / Dlow,
             Dlow = max(sum max(w - dW, 0), B3[2]^2) <= sum w' <= Dhigh = sum (w + dW).
      var    (sum max(w - dW, 0)^2 max(var_q - Av_q, 0)) / Dhigh^2 <= var' <= (sum (w + dW)^2 (var_q + Av_q)) / Dlow^2, each
             side widened by 30 u and 1e-30 (float32 underflow of w w var): Av' is the larger distance.
    The last iteration's product with the albedo adds u |out|.  The bounds are finite wherever the inputs are."""
    c = np.asarray(hist, np.float64)
    var = np.asarray(var, np.float64).copy()
    H, W = var.shape
    if iterations == 0:
        return c.copy(), var, np.zeros((H, W, 3)), np.zeros((H, W))
    a = np.asarray(features, np.float64)[..., 0:3]
    u = demodulate(c, features)
    E = 2 * U32 * np.abs(u)
    Av = np.zeros((H, W))
    guided = not np.isinf(sigma_color)
    with np.errstate(all="ignore"):
        for k in range(iterations):
            s = 2 ** k
            Lp = A.luma(u); ELp = A.luma(E)
            if guided:
                gv = blur3(var)
                Agv = blur3(Av) + 11 * U32 * gv
                lden = sigma_color * np.sqrt(gv) + 1e-4
                hi = sigma_color * np.sqrt(gv + Agv) + 1e-4
                lo = sigma_color * np.sqrt(np.maximum(gv - Agv, 0.0)) + 1e-4
                el = np.maximum(np.log(hi / lden), np.log(lden / lo)) + 5 * U32
            taps = []
            for j in range(-2, 3):
                for i in range(-2, 3):
                    uq, valid = A.tap(u, j * s, i * s)
                    vq, _ = A.tap(var, j * s, i * s)
                    Eq, _ = A.tap(E, j * s, i * s)
                    Avq, _ = A.tap(Av, j * s, i * s)
                    wn, wz, _ = edge_weight(features, j * s, i * s, s, sigma_normal, sigma_depth)
                    w = B3[i + 2] * B3[j + 2] * valid
                    dt = np.zeros((H, W))
                    centre = (i, j) == (0, 0)
                    if guided:
                        Lq = A.luma(uq)
                        x = np.abs(Lp - Lq) / lden
                        w = w * np.exp(-x)
                        if not centre:
                            dt = dt + ((ELp + A.luma(Eq) + 3 * U32 * (np.abs(Lp) + np.abs(Lq))) / lden) * np.exp(el) + x * (np.expm1(el) + 8 * U32)
                    if sigma_normal != 0 and not centre:
                        w = w * wn
                        dt = dt + 20 * U32 * sigma_normal
                    if not np.isinf(sigma_depth):
                        w = w * wz
                        if not centre:
                            dt = dt + 264 * U32
                    w = np.where(valid, w, 0.0)
                    dW = np.where(valid, (0.0 if centre else w * np.expm1(dt + 6 * U32) + 1e-36), 0.0) + np.zeros((H, W))
                    cap = B3[i + 2] * B3[j + 2]  # 0 <= w' <= B3 B3: wl, wn, wz are at most 1 on both sides
                    dW = np.where(valid, np.minimum(np.where(np.isnan(dW), np.inf, dW), np.maximum(cap - w, w)), 0.0)
                    taps.append((w, dW, uq, vq, Eq, Avq))
            den = sum(t[0] for t in taps)
            num = sum(t[0][..., None] * np.where(t[0][..., None] > 0, t[2], 0.0) for t in taps)
            out = num / den[..., None]
            vout = sum(t[0] * t[0] * np.where(t[0] > 0, t[3], 0.0) for t in taps) / (den * den)
            Dlow = np.maximum(sum(np.maximum(t[0] - t[1], 0.0) for t in taps), B3[2] * B3[2])
            Dhigh = sum(t[0] + t[1] for t in taps)
            En = np.zeros((H, W, 3)); vhi = np.zeros((H, W)); vlo = np.zeros((H, W))
            for w, dW, uq, vq, Eq, Avq in taps:
                live = (w + dW) > 0
                uq = np.where(live[..., None], uq, 0.0); Eq = np.where(live[..., None], Eq, 0.0)
                vq = np.where(live, vq, 0.0); Avq = np.where(live, Avq, 0.0)
                wh = (w + dW)[..., None]
                En += dW[..., None] * np.abs(uq - out) + wh * Eq + 27 * U32 * wh * (np.abs(uq) + Eq)
                vhi += (w + dW) ** 2 * (vq + Avq)
                vlo += np.maximum(w - dW, 0.0) ** 2 * np.maximum(vq - Avq, 0.0)
            E = En / Dlow[..., None]
            vhi = vhi / (Dlow * Dlow) * (1 + 30 * U32) + 1e-30
            vlo = vlo / (Dhigh * Dhigh) * (1 - 30 * U32) - 1e-30
            Av = np.maximum(vhi - vout, vout - vlo)
            E = np.where(np.isfinite(E), E, np.inf); Av = np.where(np.isfinite(Av), Av, np.inf)
            u, var = out, vout
        res = np.ones(c.shape)
        res[..., :3] = a * u
        Eo = a * E + U32 * np.abs(res[..., :3])
    return res, var, Eo, Av


def svgf(hist, moments, features, n, iterations=4, sigma_color=8.0, sigma_normal=32.0, sigma_depth=0.05):
    """fspt_svgf_eval: (out, v, var_K, scale)."""
    v, scale = variance(hist, moments, features, n, sigma_normal, sigma_depth)
    out, vk = guided_atrous(hist, v, features, iterations, sigma_color, sigma_normal, sigma_depth)
    return out, v, vk, scale


def synthetic_history(H, W, seed=0, n=2, floor=False):
    """hist, moments, features for fspt_svgf_eval from atrous_inputs.synthetic's accumulator and features: history lengths
    on both sides of 4 n (including 0 < Fe < 1 and exactly 4), moments of l = L(u) with a variance that is exactly 0 on a
    part of the frame (M2 = M1 M1 in float32 where the product is exact: l rounded to 12 bits) and huge (up to 1e12
    relative to the mean) on another.  floor=True: the same lengths, and a per-frame standard deviation of 20-60 % of the
    mean everywhere (no zero, no huge variance) - the set on which the variance-guided weight stays well conditioned."""
    import atrous_inputs as I
    acc, f = I.synthetic(H, W, seed)
    rng = np.random.default_rng([seed, H, W, 9])
    hist = acc.copy()
    lengths = np.array([0.5, 1, 2, 3, 3.5, 4, 5, 8, 64], np.float64) * n
    blocks = rng.integers(0, len(lengths), (-(-H // 8), -(-W // 8)))
    hist[..., 3] = np.repeat(np.repeat(lengths[blocks], 8, 0), 8, 1)[:H, :W]
    l = A.luma(demodulate(acc, f))
    kind = rng.choice(3, size=(H, W), p=[0.3, 0.6, 0.1])
    # 12-bit mantissa: the square is exact in float32, so M2 - M1 M1 is exactly 0 on both sides
    m1 = l.astype(np.float32)
    m1_12 = (m1.view(np.uint32) & np.uint32(0xFFFFF000)).view(np.float32)
    M1 = np.where(kind == 0, m1_12, m1).astype(np.float32)
    rel = np.where(kind == 0, 0.0, np.where(kind == 1, rng.uniform(0.0, 0.5, (H, W)) ** 2, 10.0 ** rng.uniform(3, 12, (H, W))))
    M2 = (M1.astype(np.float64) ** 2 * (1.0 + rel) + np.where(kind == 2, 1.0, 0.0) * rel).astype(np.float32)
    M2 = np.where(kind == 0, M1 * M1, M2).astype(np.float32)
    if floor:
        M1 = m1
        M2 = (M1.astype(np.float64) ** 2 * (1.0 + rng.uniform(0.2, 0.6, (H, W)) ** 2)).astype(np.float32)
    return hist.astype(np.float32), np.stack([M1, M2], -1).astype(np.float32), f
