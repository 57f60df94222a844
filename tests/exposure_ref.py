"""Auto-exposure restated: the binning in numpy uint32 arithmetic on the float32 luma, the resolve in float64.

The luma is k_draw's own, fma(b, 0.0722, fma(g, 0.7152, r 0.2126)) in float32.  temporal_ref.fma32 rounds twice (to float64,
then to float32), which differs from a real fma about once in 2^29 operands; a histogram of two million pixels is compared bit
for bit, so the sum is rounded to ODD in float64 here (Boldo / Melquiond: with 53 >= 2 x 24 + 2 bits the second rounding then
gives the correctly rounded float32), which makes the restatement exact.  The histogram is integer work on those bits: no
tolerance.  The resolve follows the kernel's operation order in float64; only log2(key) and exp2(e) go through a library
function on either side.
"""
import numpy as np

F = np.float32
BINS = 256
MIN_L = F(2.0 ** -16)
DEFAULTS = {"key": 0.18, "low": 0.10, "high": 0.90, "adapt_up": 1.0, "adapt_down": 1.0, "min_log2": -8.0, "max_log2": 8.0}
# log2(1 + (m + 0.5) / 8), m = 0..7: the same double literals as the kernel's
SUB = (0.0874628412503394, 0.2479275134435855, 0.3923174227787603, 0.5235619560570128, 0.6438561897747247, 0.7548875021634686,
       0.8579809951275721, 0.9541963103868752)
FIRST = {"exposure": F(1.0), "valid": 0, "metered": 0, "log2_exposure": 0.0, "log2_mean": 0.0}  # never metered


def fma32(a, b, c):
    """float32 fma, exact: the product is exact in float64, the sum is rounded to odd there, then once to float32"""
    with np.errstate(invalid="ignore", over="ignore"):
        p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
        c = np.broadcast_to(np.asarray(c, np.float64), p.shape)
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & (err != 0.0) & ((s.view(np.int64) & 1) == 0)
        away = (err > 0.0) == (s > 0.0)  # the exact sum lies further from zero than s: the next magnitude up is the odd neighbour
        bits = s.view(np.int64) + np.where(fix, np.where(away, 1, -1), 0)
        return bits.view(np.float64).astype(F)


def luma(rgba):
    rgba = np.asarray(rgba, F)
    r, g, b = rgba[..., 0], rgba[..., 1], rgba[..., 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return fma32(b, F(0.0722), fma32(g, F(0.7152), (r * F(0.2126)).astype(F)))


def bins_of(L):
    """bin per value (int64), -1 = left out"""
    L = np.asarray(L, F)
    with np.errstate(invalid="ignore"):
        keep = L >= MIN_L  # (False for NaN)
    b = (L.view(np.uint32) >> np.uint32(20)).astype(np.int64) - ((127 - 16) << 3)
    return np.where(keep, np.minimum(b, 255), -1)


def histogram(rgba, viewport=None):
    """uint32 [256] over the viewport (vw, vh) of rgba [H, W, 4]"""
    rgba = np.asarray(rgba, F)
    if viewport is not None:
        rgba = rgba[:viewport[1], :viewport[0]]
    b = bins_of(luma(rgba)).reshape(-1)
    return np.bincount(b[b >= 0], minlength=BINS).astype(np.uint32)


def bin_value(b):
    return float((b >> 3) - 16) + SUB[b & 7]


def params32(**params):
    """the parameters as the library holds them: float32, widened"""
    unknown = set(params) - set(DEFAULTS)
    assert not unknown, unknown
    return {k: float(F(v)) for k, v in {**DEFAULTS, **params}.items()}


def resolve(hist, prev=None, **params):
    """the state k_exposure_resolve leaves (a dict like FIRST), from the counts and the previous state (None: never metered)"""
    p = params32(**params)
    prev = dict(FIRST if prev is None else prev)
    N = int(np.asarray(hist, np.uint64).sum())
    if N == 0:
        return prev
    r0, r1 = int(np.floor(p["low"] * float(N))), int(np.ceil(p["high"] * float(N)))
    at, K, s = 0, 0, 0.0
    for b in range(BINS):
        c = int(hist[b])
        lo, hi = max(at, r0), min(at + c, r1)
        at += c
        if hi <= lo:
            continue
        s += float(hi - lo) * bin_value(b)
        K += hi - lo
    mean = s / float(K)
    target = float(np.log2(np.float64(p["key"]))) - mean
    e = target
    if prev["valid"]:
        q = float(prev["log2_exposure"])
        e = q + (target - q) * (p["adapt_up"] if target < q else p["adapt_down"])
    e = min(max(e, p["min_log2"]), p["max_log2"])
    return {"exposure": F(np.exp2(np.float64(e))), "valid": 1, "metered": N, "log2_exposure": e, "log2_mean": mean}


def meter(rgba, viewport=None, prev=None, **params):
    h = histogram(rgba, viewport)
    return h, resolve(h, prev, **params)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def rgb_for_luma(L):
    """float32 (r, g, 0) [n, 3] whose luma is L exactly: r x 0.2126f carries about half of L, and g, which then lies in L's binade
    or the one below, moves the fma's exact sum in steps of at most 0.72 ulp of L, so one of the g next to (L - c) / 0.7152f
    rounds to L"""
    L = np.asarray(L, F)
    r = (L.astype(np.float64) * 0.5 / np.float64(F(0.2126))).astype(F)
    c = (r * F(0.2126)).astype(F)
    g0 = ((L.astype(np.float64) - c.astype(np.float64)) / np.float64(F(0.7152))).astype(F)
    out = np.full(L.shape, np.nan, F)
    up, dn = g0.copy(), g0.copy()
    for _ in range(4):  # g0, then outwards
        for g in (up, dn):
            hit = np.isnan(out) & (fma32(g, F(0.7152), c) == L)
            out[hit] = g[hit]
        up, dn = np.nextafter(up, F(np.inf)), np.nextafter(dn, F(-np.inf))
    assert not np.isnan(out).any()
    return np.stack([r, out, np.zeros_like(r)], -1)


def edge_lumas():
    """every bin edge 2^e (1 + m / 8), e = -16..15, m = 0..7, then 2^16, and the floats one ulp either side of each: 771 values"""
    e = np.arange(-16, 16, dtype=np.float64)[:, None]
    edges = np.append((2.0 ** e * (1.0 + np.arange(8) / 8.0)).reshape(-1), 2.0 ** 16).astype(F)
    return np.concatenate([np.nextafter(edges, F(0)), edges, np.nextafter(edges, F(np.inf))])


def image(W, H, kind, seed=7):
    """the GPU tests' inputs, float32 [H, W, 4] (.w = 1)"""
    rng = np.random.default_rng(seed + 131 * W + H)
    img = np.zeros((H, W, 4), F)
    img[..., 3] = 1.0
    n = W * H
    flat = img.reshape(-1, 4)
    if kind == "constant":  # one bin for the whole frame: the contention case
        flat[:, :3] = F([0.5, 0.25, 0.75])
    elif kind == "edges":  # lumas exactly on the edges and one ulp beside them, tiled over the frame
        Ls = edge_lumas()
        flat[:, :3] = rgb_for_luma(Ls)[np.arange(n) % Ls.size]
    elif kind == "special":  # what is left out, and what saturates
        vals = F([0.0, -0.0, -1.0, -1e30, np.nan, np.inf, -np.inf, 1e-45, 1e-39, 1.1754942e-38, 2.0 ** -17, 2.0 ** -16, 65535.0, 65536.0, 1e5, 3e38, 1.0])
        flat[:, :3] = vals[rng.integers(0, vals.size, (n, 3))]
        flat[::3, 1:3] = 0.0  # (a lone channel keeps its special value: inf + -inf would only make more NaN)
    elif kind == "noise":  # log-uniform over 30 octaves
        flat[:, :3] = (2.0 ** rng.uniform(-15.0, 15.0, (n, 3))).astype(F)
    elif kind == "excluded":  # not one pixel counts
        vals = F([0.0, -2.0, np.nan, 1e-40, 2.0 ** -18])
        flat[:, :3] = vals[rng.integers(0, vals.size, (n, 1))]
    else:
        raise ValueError(kind)
    return img


KINDS = ("constant", "edges", "special", "noise", "excluded")
SHAPES = [(1, 1), (3, 2), (16, 16), (17, 33), (50, 37)]
BIG_SHAPE = (1920, 1080)
# the mean's error from the operation count: 256 products and sums in double with |v| <= 16, and the division
GAMMA_BOUND = 258 * 2.0 ** -53 / (1 - 258 * 2.0 ** -53) * 16.0
MEAN_TOL = 1e-9  # absolute; the slack above GAMMA_BOUND (4.6e-13) only covers the device's double log2 / exp2


def ulp_diff32(a, b):
    """distance of two positive finite float32 in ulps"""
    return abs(int(np.asarray(a, F).view(np.int32)) - int(np.asarray(b, F).view(np.int32)))
