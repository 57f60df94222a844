"""float64 numpy restatement of the guided a-trous filter of fspt_denoise (include/fspt.h): the checker the
GPU tests compare the HIP kernel against.  accum: (H, W, 4), features: (H, W, 8) = albedo.rgb, depth, normal.xyz,
coverage - the library's layout and row order."""
import numpy as np

B3 = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0


def luma(u):
    return 0.2126 * u[..., 0] + 0.7152 * u[..., 1] + 0.0722 * u[..., 2]


def tap(arr, dy, dx):
    """arr at q = p + (dy, dx) for every p, and where q lies inside the image."""
    H, W = arr.shape[:2]
    ys = np.arange(H)[:, None] + dy
    xs = np.arange(W)[None, :] + dx
    valid = (ys >= 0) & (ys < H) & (xs >= 0) & (xs < W)
    return arr[np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)], valid


def atrous(accum, features, iterations=4, sigma_color=4.0, sigma_normal=32.0, sigma_depth=0.05):
    """Defaults: the library's (include/fspt.h FSPT_DENOISE_*)."""
    c = np.asarray(accum, np.float64)
    f = np.asarray(features, np.float64)
    if iterations == 0:
        return c.copy()
    a, z, n, h = f[..., 0:3], f[..., 3], f[..., 4:7], f[..., 7]
    nlen = np.sqrt((n * n).sum(-1))
    u = c[..., :3] / np.maximum(a, 1e-3)
    for k in range(iterations):
        s = 2 ** k
        Lp = luma(u)
        num = np.zeros_like(u)
        den = np.zeros(u.shape[:2])
        for j in range(-2, 3):
            for i in range(-2, 3):
                uq, valid = tap(u, j * s, i * s)
                zq, _ = tap(z, j * s, i * s)
                nq, _ = tap(n, j * s, i * s)
                hq, _ = tap(h, j * s, i * s)
                lq, _ = tap(nlen, j * s, i * s)
                w = B3[i + 2] * B3[j + 2] * valid
                if not np.isinf(sigma_color):
                    Lq = luma(uq)
                    w = w * np.exp(-np.abs(Lp - Lq) / (sigma_color * 2.0 ** -k * (Lp + Lq) + 1e-4))
                if sigma_normal != 0 and (i, j) != (0, 0):
                    both_miss = (h == 0) & (hq == 0)
                    cut = ((h == 0) != (hq == 0)) | (nlen == 0) | (lq == 0)
                    with np.errstate(invalid="ignore", divide="ignore"):
                        cos = (n * nq).sum(-1) / (nlen * lq)
                        wn = np.maximum(0.0, np.where(cut, 0.0, cos)) ** sigma_normal
                    w = w * np.where(both_miss, 1.0, np.where(cut, 0.0, wn))
                if not np.isinf(sigma_depth):
                    w = w * np.exp(-np.abs(z - zq) / (sigma_depth * s * np.maximum(z, 1e-3)))
                num += w[..., None] * uq
                den += w
        u = num / den[..., None]
    out = np.ones(c.shape)
    out[..., :3] = a * u
    return out
