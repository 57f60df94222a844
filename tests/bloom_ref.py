"""Bloom restated in float64, in the order include/fspt_tuning.h fixes, with the error bound that order gives.

Every function takes and returns float64 arrays [h, w, 3] (the .w channel takes no part).  The kernels do the same operations
in float32; `pyramid` therefore also runs the recursion on MAGNITUDES (every weight is positive and every sanitised input is
>= 0, so the D levels are their own magnitudes; the combine's difference `up - D` is bounded by `up + D`) and counts the
roundings on the deepest path to each quantity:

    one 1-D down pass   a1 + a2 | its product by 3 | a0 + a3 | their sum      3 deep (the product by 1/8 is exact)
    D_k                 two passes per level                                   6 k
    up(U)               fma(3/4, fma(3/4, a, b / 4), fma(3/4, c, d / 4) / 4)   2 deep
    U_n = D_n                                                                  6 n
    U_k, k < n          up, the difference, the fma                            6 n + 4 (n - k)
    B = up(U_1)                                                                10 n - 2
    c' = fma(i, B - c0, c0)                                                    10 n

so |float32 result - float64 result| <= gamma(m) x magnitude + absolute term, gamma(m) = m u / (1 - m u), u = 2^-24.  The
absolute term covers results below the smallest normal float32, where a rounding (gradual underflow) or a flush to zero loses
up to 2^-126 whatever the magnitude: ETA per rounding or scaling on the path, carried through the recursion as a scalar (the
weights of every step sum to 1; the combine at most triples it).  The float64 recursion's own error, gamma_64(m) x magnitude,
is added as well; it is 2^-29 of the float32 term.  Nothing here was fitted to what the kernels give.
"""
import numpy as np

F = np.float32
CLAMP = 1024.0
MAX_LEVELS = 8
DEFAULTS = {"intensity": 0.05, "scatter": 0.7, "levels": 6}
TAIL_TEXELS = 2048
U32, U64 = 2.0 ** -24, 2.0 ** -53
ETA = 2.0 ** -126


def gamma(m, u=U32):
    return m * u / (1.0 - m * u)


def sanitise(v):
    """s(v) = v >= 0 ? min(v, CLAMP) : 0 (NaN and negatives: 0, +inf: the clamp)"""
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(v >= 0.0, np.minimum(v, CLAMP), 0.0)


def sizes(vw, vh, levels=DEFAULTS["levels"]):
    """[(w_1, h_1) .. (w_n, h_n)]: w_{k+1} = (w_k + 1) >> 1; n = min(levels, the first k with min(w_k, h_k) == 1)"""
    out, w, h = [], int(vw), int(vh)
    while len(out) < levels and min(w, h) > 1:
        w, h = (w + 1) >> 1, (h + 1) >> 1
        out.append((w, h))
    return out


def down_pass(a, axis):
    """one 1-D pass of w = (1, 3, 3, 1) / 8 along `axis`, taps clamped: ((a1 + a2) 3 + (a0 + a3)) / 8"""
    n = a.shape[axis]
    x = np.arange((n + 1) >> 1)
    t = [np.take(a, np.clip(2 * x - 1 + i, 0, n - 1), axis=axis) for i in range(4)]
    return ((t[1] + t[2]) * 3.0 + (t[0] + t[3])) * 0.125


def down(S):
    """D_{k+1} from S_k [h, w, 3]: horizontal first"""
    return down_pass(down_pass(S, 1), 0)


def tent_taps(nf, nc):
    """for fine coordinates 0 .. nf - 1 over a coarse level of nc: (c0, c1), weights 3/4 and 1/4"""
    x = np.arange(nf)
    c0 = x >> 1
    c1 = np.clip(c0 + np.where(x & 1, 1, -1), 0, nc - 1)
    return c0, c1


def up(U, wf, hf):
    """up(U) at a fine level of wf x hf: the 2 x 2 tent, horizontal first"""
    h, w = U.shape[:2]
    cx0, cx1 = tent_taps(wf, w)
    cy0, cy1 = tent_taps(hf, h)
    t = 0.75 * U[:, cx0] + 0.25 * U[:, cx1]
    return 0.75 * t[cy0] + 0.25 * t[cy1]


def params32(**params):
    """the parameters as the library holds them: float32, widened"""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    p = {**DEFAULTS, **params}
    return float(F(p["intensity"])), float(F(p["scatter"])), int(p["levels"])


def pyramid(rgba, viewport=None, **params):
    """rgba float32 [H, W, 4] -> a dict: n; down, up = the lists D_1 .. D_n, U_1 .. U_n [h_k, w_k, 3]; bloom = B [vh, vw, 3];
    mix = c' [H, W, 3] (the source outside the viewport and with n = 0, as the draw draws it plain); and under the same keys
    with `_tol` appended the bound on |float32 kernel - this| per texel (0 where nothing is computed)."""
    intensity, scatter, levels = params32(**params)
    rgba = np.asarray(rgba, F)
    H, W = rgba.shape[:2]
    vw, vh = (W, H) if viewport is None else viewport
    src = rgba[..., :3].astype(np.float64)
    lv = sizes(vw, vh, levels)
    n = len(lv)
    out = {"n": n, "sizes": lv}
    if n == 0:
        out.update(down=[], up=[], bloom=src[:vh, :vw].copy(), mix=src.copy(), down_tol=[], up_tol=[],
                   bloom_tol=np.zeros((vh, vw, 3)), mix_tol=np.zeros((H, W, 3)))
        return out
    c0 = sanitise(src[:vh, :vw])
    D = [c0]
    for _ in range(n):
        D.append(down(D[-1]))
    tol = lambda m, mag, a: (gamma(m) + gamma(m, U64)) * mag + a
    aD = [10 * k * ETA for k in range(n + 1)]  # (4 roundings and a scaling per pass)
    out["down"], out["down_tol"] = D[1:], [tol(6 * k, D[k], aD[k]) for k in range(1, n + 1)]
    # U and its magnitude M; the scalar absolute term a
    U, M, a = [None] * (n + 1), [None] * (n + 1), [0.0] * (n + 1)
    U[n], M[n], a[n] = D[n], D[n], aD[n]
    for k in range(n - 1, 0, -1):
        w, h = lv[k - 1]
        u, m = up(U[k + 1], w, h), up(M[k + 1], w, h)
        U[k] = scatter * (u - D[k]) + D[k]
        M[k] = scatter * (m + D[k]) + D[k]
        a[k] = (a[k + 1] + 6 * ETA) + 2 * aD[k] + 2 * ETA
    out["up"] = U[1:]
    out["up_tol"] = [tol(6 * n + 4 * (n - k), M[k], a[k]) for k in range(1, n + 1)]
    B, MB = up(U[1], vw, vh), up(M[1], vw, vh)
    out["bloom"], out["bloom_tol"] = B, tol(10 * n - 2, MB, a[1] + 6 * ETA)
    mix, mix_tol = src.copy(), np.zeros((H, W, 3))
    mix[:vh, :vw] = intensity * (B - c0) + c0
    mix_tol[:vh, :vw] = tol(10 * n, intensity * (MB + c0) + c0, a[1] + 8 * ETA)
    out["mix"], out["mix_tol"] = mix, mix_tol
    return out


# ---- inputs ------------------------------------------------------------------------------------------------------------------
KINDS = ("constant", "corner", "edge", "centre", "tile", "noise", "zeros", "special")
SHAPES = [(1, 1), (2, 2), (3, 2), (5, 7), (16, 16), (17, 33), (50, 37), (131, 67)]
BIG_SHAPE = (1920, 1080)
VIEWPORTS = [((50, 37), (23, 19)), ((131, 67), (65, 66)), ((17, 33), (17, 5))]


def image(W, H, kind, seed=11):
    """the tests' inputs, float32 [H, W, 4] (.w = 1)"""
    rng = np.random.default_rng(seed + 131 * W + H)
    img = np.zeros((H, W, 4), F)
    img[..., 3] = 1.0
    if kind == "constant":  # dyadic: every level is the same constant, exactly
        img[..., :3] = F([0.5, 0.25, 3.0])
    elif kind == "corner":
        img[0, 0, :3] = F([512.0, 1.0, 0.125])
    elif kind == "edge":
        img[H // 2, W - 1, :3] = F([3.0, 40.0, 0.75])
    elif kind == "centre":
        img[H // 2, W // 2, :3] = F([30.0, 30.0, 300.0])
    elif kind == "tile":  # the first source texel of the second tile of k_bloom_down (32 x 8 outputs: 64 x 16 sources), and its neighbour
        x, y = min(64, W - 1), min(16, H - 1)
        img[y, x, :3] = F([7.0, 1.0, 100.0])
        img[max(y - 1, 0), max(x - 1, 0), :3] += F([1.0, 9.0, 2.0])
    elif kind == "noise":  # log-uniform over 20 octaves
        img[..., :3] = (2.0 ** rng.uniform(-10.0, 10.0, (H, W, 3))).astype(F)
    elif kind == "zeros":
        pass
    elif kind == "special":  # what the sanitiser is for, among ordinary values
        vals = F([np.nan, np.inf, -np.inf, -1.0, -1e30, 1e-45, 1e-39, 1.1754942e-38, 1023.9999, 1024.0, 1025.0, 3e38, 0.0, 1.0, 0.3])
        img[..., :3] = vals[rng.integers(0, vals.size, (H, W, 3))]
    else:
        raise ValueError(kind)
    return img
