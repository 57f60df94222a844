"""float64 restatement of fspt_render_adaptive's estimator and schedule (include/fspt.h).

`schedule` takes the uniform frames I_R, I_2R, ..., I_max (ordinary render() results of one seed: frames[n] = the
accumulator after n ticks, rows bottom-up) and returns every tile's retired count and retiring error E_T, with the
tiles whose E_T came within `tie` (relative) of the threshold at one of their decision points marked: float32 against
float64 arithmetic may decide those either way."""
import numpy as np


def decision_splits(max_ticks, round_ticks):
    """The (m, n) pairs the schedule estimates at, in order (every round after the first; the snapshot after m ticks)."""
    out, m = [], round_ticks
    for n in range(2 * round_ticks, max_ticks + 1, round_ticks):
        out.append((m, n))
        if n >= 2 * m:
            m = n
    return out


def variance_estimate(I, S, m, n):
    """v = (B - S)^2 m (n - m) / n^2 with B = (n I - m S) / (n - m), the mean of samples m+1..n: unbiased for Var(I_n)."""
    I = np.asarray(I, np.float64); S = np.asarray(S, np.float64)
    B = (n * I - m * S) / (n - m)
    return (B - S) ** 2 * (m * (n - m)) / float(n * n)


def rel_mse_terms(I, S, m, n):
    """r = v / (I^2 + 0.01) per pixel and channel."""
    I = np.asarray(I, np.float64)
    return variance_estimate(I, S, m, n) / (I * I + 0.01)


def tile_means(r, tile, vw, vh):
    """Mean of r [H, W, 3] over each tile's pixels inside the viewport and its 3 channels -> [tiles_y, tiles_x] (NaN: no pixel)."""
    H, W = r.shape[:2]
    tx, ty = (W + tile - 1) // tile, (H + tile - 1) // tile
    pad = np.zeros((ty * tile, tx * tile, 3), np.float64)
    pad[:vh, :vw] = r[:vh, :vw]
    sums = pad.reshape(ty, tile, tx, tile, 3).sum(axis=(1, 3, 4))
    inside = np.zeros((ty * tile, tx * tile), np.float64)
    inside[:vh, :vw] = 1.0
    npx = inside.reshape(ty, tile, tx, tile).sum(axis=(1, 3))
    with np.errstate(invalid="ignore", divide="ignore"):
        return sums / (3.0 * npx)


def active_tiles(W, H, tile, vw, vh):
    tx, ty = (W + tile - 1) // tile, (H + tile - 1) // tile
    gx, gy = np.meshgrid(np.arange(tx) * tile, np.arange(ty) * tile)
    return (gx < vw) & (gy < vh)


def schedule(frames, target, max_ticks=1024, min_ticks=64, round_ticks=32, tile=32, viewport=None, tie=1e-4):
    """-> (counts [ty, tx] uint32, err [ty, tx] float64, tied [ty, tx] bool, rounds)."""
    R = round_ticks
    first = np.asarray(frames[R])
    H, W = first.shape[:2]
    vw, vh = viewport if viewport else (W, H)
    active = active_tiles(W, H, tile, vw, vh)
    counts = np.zeros(active.shape, np.uint32)
    err = np.zeros(active.shape, np.float64)
    tied = np.zeros(active.shape, bool)
    S, m, rounds = None, 0, 0
    for n in range(R, max_ticks + 1, R):
        if not active.any():
            break
        rounds += 1
        I = np.asarray(frames[n], np.float64)[..., :3]
        if m == 0:
            S, m = I.copy(), n
            continue
        decide, refresh = n >= min_ticks, n >= 2 * m
        if decide:
            E = tile_means(rel_mse_terms(I, S, m, n), tile, vw, vh)
            with np.errstate(invalid="ignore"):
                retire = active & ((n >= max_ticks) | (E < target))
                tied |= active & (np.abs(E - target) <= tie * target) & (n < max_ticks)
            counts[retire] = n
            err[retire] = E[retire]
            active &= ~retire
        if refresh:
            S, m = I.copy(), n
    return counts, err, tied, rounds


def expand(counts, W, H, tile=32, viewport=None):
    """Per-tile counts -> per-pixel [H, W] (0 outside the viewport), as fspt_read_sample_counts."""
    vw, vh = viewport if viewport else (W, H)
    px = np.repeat(np.repeat(counts, tile, axis=0), tile, axis=1)[:H, :W].copy()
    px[vh:, :] = 0
    px[:, vw:] = 0
    return px
