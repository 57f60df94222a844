"""float64 numpy restatement of the guided a-trous filter of fspt_denoise (include/fspt.h): the checker the
GPU tests compare the HIP kernel against.  accum: (H, W, 4), features: (H, W, 8) = albedo.rgb, depth, normal.xyz,
coverage - the library's layout and row order.

`mutant` names one deliberate defect (MUTANTS) for tests/test_denoise_cpu.py, which proves that the test inputs
(tests/atrous_inputs.py) tell each of them from the filter as defined; None is the filter itself."""
import numpy as np

B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0

MUTANTS = (
    "clamp_taps",          # taps outside the image read the edge pixel instead of being dropped
    "sigma_color_up",      # sigma_color scaled by 2^k instead of 2^-k
    "depth_unscaled",      # sigma_depth not scaled by the step
    "step_doubled",        # step 2^(k+1) instead of 2^k
    "normal_at_centre",    # the normal weight applied at the centre tap too
    "no_hit_miss_cut",     # no cut between a hit and a miss (only the zero-length-normal cut left)
    "miss_pairs_zero",     # two misses weigh 0 instead of 1
    "full_coverage_only",  # a pixel counts as a hit only when its coverage is exactly 1
    "no_albedo_floor",     # u = c / a without the 1e-3 floor
    "rec601_luma",         # Rec.601 luma weights instead of Rec.709
    "depth_floor_q",       # the depth floor taken from z_q instead of z_p
)


def luma(u, rec601=False):
    if rec601:
        return 0.299 * u[..., 0] + 0.587 * u[..., 1] + 0.114 * u[..., 2]
    return 0.2126 * u[..., 0] + 0.7152 * u[..., 1] + 0.0722 * u[..., 2]


def tap(arr, dy, dx):
    """arr at q = p + (dy, dx) for every p, and where q lies inside the image."""
    H, W = arr.shape[:2]
    ys = np.arange(H)[:, None] + dy
    xs = np.arange(W)[None, :] + dx
    valid = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    return arr[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], valid


def atrous(accum, features, iterations=4, sigma_color=4.0, sigma_normal=32.0, sigma_depth=0.05, *, mutant=None):
    """Defaults: the library's (include/fspt.h FSPT_DENOISE_*)."""
    assert mutant is None or mutant in MUTANTS, mutant
    m = mutant
    c = np.asarray(accum, np.float64)
    f = np.asarray(features, np.float64)
    if iterations == 0:
        return c.copy()
    a, z, n, h = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7]
    hit = (h == 1) if m == "full_coverage_only" else (h != 0)
    nlen = np.sqrt((n * n).sum(-1))
    with np.errstate(invalid="ignore", divide="ignore"):
        u = c[..., :3] / (a if m == "no_albedo_floor" else np.maximum(a, 1e-3))
    for k in range(iterations):
        s = 2 ** (k + 1) if m == "step_doubled" else 2 ** k
        Lp = luma(u, m == "rec601_luma")
        num = np.zeros_like(u)
        den = np.zeros(u.shape[:2])
        for j in range(-2, 3):
            for i in range(-2, 3):
                uq, valid = tap(u, j * s, i * s)
                zq, _ = tap(z, j * s, i * s)
                nq, _ = tap(n, j * s, i * s)
                hq, _ = tap(hit, j * s, i * s)
                lq, _ = tap(nlen, j * s, i * s)
                w = B3[i + 2] * B3[j + 2] * (True if m == "clamp_taps" else valid)
                if not np.isinf(sigma_color):
                    Lq = luma(uq, m == "rec601_luma")
                    sc = sigma_color * 2.0 ** (k if m == "sigma_color_up" else -k)
                    with np.errstate(invalid="ignore"):
                        w = w * np.exp(-np.abs(Lp - Lq) / (sc * (Lp + Lq) + 1e-4))
                if sigma_normal != 0 and ((i, j) != (0, 0) or m == "normal_at_centre"):
                    both_miss = ~hit & ~hq
                    cut = (nlen == 0) | (lq == 0)
                    if m != "no_hit_miss_cut":
                        cut |= hit != hq
                    with np.errstate(invalid="ignore", divide="ignore"):
                        # the cosine clamped to 1: float32 rounding may put it above (include/fspt.h)
                        cos = np.minimum((n * nq).sum(-1) / (nlen * lq), 1.0)
                        wn = np.maximum(0.0, np.where(cut, 0.0, cos)) ** sigma_normal
                    w = w * np.where(both_miss, 0.0 if m == "miss_pairs_zero" else 1.0, np.where(cut, 0.0, wn))
                if not np.isinf(sigma_depth):
                    zs = sigma_depth * (1 if m == "depth_unscaled" else s) * np.maximum(zq if m == "depth_floor_q" else z, 1e-3)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        w = w * np.where(z == zq, 1.0, np.exp(-np.abs(z - zq) / zs))  # equal depths weigh 1
                with np.errstate(invalid="ignore"):
                    num += w[..., None] * uq
                den += w
        with np.errstate(invalid="ignore", divide="ignore"):
            u = num / den[..., None]
    out = np.ones(c.shape)
    out[..., :3] = a * u
    return out
