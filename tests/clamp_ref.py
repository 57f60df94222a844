"""float64 restatement of the temporal history clamp (include/fspt_tuning.h), the bounds the GPU tests hold
k_temporal_clamp to, and the synthetic inputs both test files share.

The fast history's own recursion needs no restatement here: it is tests/temporal_ref.py's blend with max_history =
fast_history, and the GPU test checks it bit for bit against a second target run that way.

clamp(hist, fast, sigma_scale): per pixel p and channel c over the taps of the 5 x 5 window around p inside the image,
  mu = sum F_c / cnt, m2 = sum F_c^2 / cnt, sd = sqrt(max(0, m2 - mu^2)), lo = mu - s sd, hi = mu + s sd,
  out_c = min(max(hist_c, lo), hi); .w untouched; s = +inf: out = hist, lo = -inf, hi = +inf (no inf * 0).
"""
import numpy as np

RADIUS = 2
U = 2.0 ** -24  # unit roundoff of float32


def window_sums(fast):
    """(cnt [H, W], S1, S2, A1 [H, W, 3]) in float64: the number of window taps inside the image, and over them the sums
    of F_c, F_c^2 and |F_c|."""
    f = np.asarray(fast, np.float64)[..., :3]
    H, W = f.shape[:2]
    r = RADIUS
    pad = np.zeros((H + 2 * r, W + 2 * r, 3))
    pad[r:r + H, r:r + W] = f
    one = np.zeros((H + 2 * r, W + 2 * r))
    one[r:r + H, r:r + W] = 1.0
    cnt = np.zeros((H, W)); s1 = np.zeros((H, W, 3)); s2 = np.zeros((H, W, 3)); a1 = np.zeros((H, W, 3))
    for j in range(2 * r + 1):
        for i in range(2 * r + 1):
            v = pad[j:j + H, i:i + W]
            cnt += one[j:j + H, i:i + W]
            s1 += v; s2 += v * v; a1 += np.abs(v)
    return cnt, s1, s2, a1


def box(fast, sigma_scale):
    """mu, sd, lo, hi [H, W, 3] (float64) and cnt [H, W]"""
    cnt, s1, s2, _ = window_sums(fast)
    mu = s1 / cnt[..., None]
    m2 = s2 / cnt[..., None]
    sd = np.sqrt(np.maximum(0.0, m2 - mu * mu))
    if np.isinf(sigma_scale):
        lo, hi = np.full_like(mu, -np.inf), np.full_like(mu, np.inf)
    else:
        lo, hi = mu - sigma_scale * sd, mu + sigma_scale * sd
    return mu, sd, lo, hi, cnt


def clamp(hist, fast, sigma_scale):
    """-> (out [H, W, 4], lo, hi [H, W, 3]) in float64"""
    h = np.asarray(hist, np.float64)
    _, _, lo, hi, _ = box(fast, sigma_scale)
    out = h.copy()
    if not np.isinf(sigma_scale):
        out[..., :3] = np.minimum(np.maximum(h[..., :3], lo), hi)
    return out, lo, hi


def gamma(k):
    """Higham's gamma_k for float32: the relative error bound of k chained roundings"""
    return k * U / (1.0 - k * U)


def tolerances(fast, sigma_scale):
    """(tol_mu, e, tol_sd, tol_box [H, W, 3]) for k_temporal_clamp's float32 arithmetic, from its operation count alone.
    The kernel sums the window's cnt taps one after the other (cnt - 1 roundings that matter: zeros outside the image add
    exactly) and divides by cnt, so  |d mu| <= gamma(cnt) A1 / cnt  (A1 = sum |F|: relative to mu for the non-negative
    values a history holds).  m2 is a chain of cnt fmas and a division: |d m2| <= gamma(cnt + 1) M2.  mu mu carries
    2 |mu| |d mu| and its own rounding: (2 gamma(cnt) + U) A^2 <= 2 gamma(cnt + 1) A^2, A = A1 / cnt.  The difference is
    rounded once more, U |m2 - mu^2| <= U (M2 + A^2).  Together the ABSOLUTE bound of the difference
        e = gamma(cnt + 2) M2 + 2 gamma(cnt + 2) A^2.
    sd inherits min(e / (2 sd), sqrt(e)); lo, hi and a clamped output are held to tol_mu + sigma_scale tol_sd."""
    cnt, _, s2, a1 = window_sums(fast)
    c = cnt[..., None]
    A, M2 = a1 / c, s2 / c
    tol_mu = gamma(c) * A
    e = gamma(c + 2) * M2 + 2.0 * gamma(c + 2) * A * A
    _, sd, _, _, _ = box(fast, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        tol_sd = np.where(sd > 0.0, np.minimum(e / (2.0 * sd), np.sqrt(e)), np.sqrt(e))
    tol_box = tol_mu if (sigma_scale == 0.0 or np.isinf(sigma_scale)) else tol_mu + sigma_scale * tol_sd
    return tol_mu, e, tol_sd, tol_box


def exempt(hist, fast, sigma_scale):
    """Boolean [H, W, 3]: the values whose branch (clamped or not) can flip - hist within the box tolerance of lo or hi in
    the restatement.  Decided from the restatement alone; the tests cap it at EXEMPT_CAP of a case's values."""
    if np.isinf(sigma_scale):
        return np.zeros(np.shape(hist)[:2] + (3,), bool)
    h = np.asarray(hist, np.float64)[..., :3]
    _, lo, hi = clamp(hist, fast, sigma_scale)
    tol = tolerances(fast, sigma_scale)[3]
    return (np.abs(h - lo) <= tol) | (np.abs(h - hi) <= tol)


EXEMPT_CAP = 0.01
SHAPES = [(1, 1), (3, 2), (5, 5), (16, 16), (17, 33), (50, 37)]  # (W, H); the GPU test adds one 1920 x 1080
BIG_SHAPE = (1920, 1080)
SIGMAS = [0.0, 1.0, 2.0, float("inf")]


def synthetic(W, H, seed=0):
    """(hist, fast) float32 [H, W, 4] for a W x H case.  fast, in vertical bands of seven columns: a constant band (exact-zero
    spread), ordinary noise (spread a third of the mean), rare spikes of 1e2 - 1e6 x the band's level, exact zeros, and a
    signed band of +-level (+ 1e-6 level) whose window mean cancels to about 1e-6 of its spread - for non-negative values
    the spread cannot exceed sqrt(24) means, so this is the band whose spread reaches 1e6 x the mean; lengths in .w.
    hist, per value: the mean +- 0.5 / 1.5 / 2.5 / 100 spreads (inside or outside, depending on sigma_scale; where the
    spread is zero, a tenth of the mean + 0.1 stands in for it, so these lie outside), 1e4 x the mean + 1 and the mean - 1000 spreads
    (far outside), and RARELY (0.5 % together, and only in a case of 200 values or more, where one such value is under
    the cap: these are the values whose branch may flip) exactly the restatement's float32 lo or hi at sigma_scale 1 or 2,
    or the mean itself."""
    rng = np.random.default_rng(1000 * seed + 31 * W + H)
    fast = np.zeros((H, W, 4), np.float32)
    band = (np.arange(W) // 7 + W % 5 + 1) % 5  # (the first band depends on W, so that the cases narrower than a band differ)
    level = rng.uniform(0.05, 4.0, 3)
    for c in range(3):
        v = np.empty((H, W))
        v[:, band == 0] = level[c]
        noisy = np.abs(level[c] * (1.0 + 0.33 * rng.standard_normal((H, W))))
        v[:, band == 1] = noisy[:, band == 1]
        spikes = np.where(rng.random((H, W)) < 0.03, level[c] * 10.0 ** rng.uniform(2, 6, (H, W)), level[c] * rng.uniform(0.9, 1.1, (H, W)))
        v[:, band == 2] = spikes[:, band == 2]
        v[:, band == 3] = 0.0
        signed = level[c] * (np.where(np.add.outer(np.arange(H), np.arange(W)) % 2 == 0, 1.0, -1.0) + 1e-6)
        v[:, band == 4] = signed[:, band == 4]
        fast[..., c] = v
    fast[..., 3] = rng.integers(1, 17, (H, W))
    mu, sd, lo1, hi1, _ = box(fast, 1.0)
    _, _, lo2, hi2, _ = box(fast, 2.0)
    spread = np.where(sd > 1e-3 * np.abs(mu), sd, 0.1 * np.abs(mu) + 0.1)
    offs = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 100.0, -100.0])
    h = mu + offs[rng.integers(0, len(offs), (H, W, 3))] * spread
    far = rng.random((H, W, 3))
    h = np.where(far < 0.05, 1e4 * mu + 1.0, h)
    h = np.where(far > 0.95, mu - 1e3 * spread, h)
    rare = rng.random((H, W, 3))
    f32 = lambda a: a.astype(np.float32).astype(np.float64)
    for k, a in enumerate((lo1, hi1, lo2, hi2, mu)):
        if W * H * 3 >= 200:
            h = np.where((rare >= 0.001 * k) & (rare < 0.001 * (k + 1)), f32(a), h)
    h = np.where((band == 3)[None, :, None], np.abs(h), h)  # (beside exact zeros only positive values are not ON the box)
    hist = np.zeros((H, W, 4), np.float32)
    hist[..., :3] = h
    hist[..., 3] = rng.integers(1, 65, (H, W))
    return hist, fast
