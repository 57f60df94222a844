"""Deterministic synthetic inputs for the guided a-trous filter (tests/atrous_ref.py, k_atrous): an accumulator and a
feature buffer in the library's layouts (H, W, 4) and (H, W, 8), made to reach every branch of the weights and every
edge of the arithmetic.  The frame is tiled with 4 x 4 blocks, each of one class:

  smooth  hits with a smoothly varying unit normal field and depth
  plane   hits sharing one plane normal (three of the four PLANES have a float32 cosine with themselves that rounds to
          1 + 2^-23) on a tilted plane whose depth jumps from block to block
  miss    h = 0, albedo 1, z = 1e5, n = 0 (what k_features writes for a pixel whose samples all missed)
  black   plane hits with black albedo (all three channels, or two): the 1e-3 demodulation floor
  zero_z  plane hits at z = 0 exactly: the 1e-3 depth floor
  stray   h = 0 with a non-zero normal: the hit / miss cut on its own (every other miss also has |n| = 0)

and per pixel: hits with a zero-length normal, seam pixels on hit blocks beside a miss block (coverage 1/4, 1/2 or 3/4;
normal, albedo and depth mixed with the miss values as k_features' means mix them), and an accumulator of gradients
and noise with exact zeros and fireflies up to 1024."""
import numpy as np

CLASSES = ("smooth", "plane", "miss", "black", "zero_z", "stray")
_P = np.array([[-0.5, 0.7, 0.2], [0.2, 0.9, 0.4], [3.0, -1.0, 2.0], [0.3, -0.2, 0.93]])
PLANES = (_P / np.linalg.norm(_P, axis=1, keepdims=True)).astype(np.float32)
BLOCK = 4
MISS = np.array([1, 1, 1, 1e5, 0, 0, 0, 0], np.float32)


def block_classes(H, W, seed=0):
    """Class index per 4 x 4 block (CLASSES), from a generator seeded by (seed, H, W)."""
    rng = np.random.default_rng([seed, H, W, 1])
    nby, nbx = -(-H // BLOCK), -(-W // BLOCK)
    return rng.choice(len(CLASSES), size=(nby, nbx), p=[0.3, 0.25, 0.2, 0.09, 0.08, 0.08])


def synthetic(H, W, seed=0):
    rng = np.random.default_rng([seed, H, W])
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    bc = block_classes(H, W, seed)
    cls = np.repeat(np.repeat(bc, BLOCK, 0), BLOCK, 1)[:H, :W]
    bid = (y // BLOCK) * 7919 + (x // BLOCK)  # block id: picks the block's plane and depth offset
    f = np.zeros((H, W, 8), np.float64)
    # smooth hits: normal field and depth varying slowly across the frame
    sm = np.stack([0.5 * np.sin(0.31 * x + 0.17 * y), 0.5 * np.cos(0.23 * y - 0.11 * x), np.ones_like(x)], -1)
    sm /= np.linalg.norm(sm, axis=-1, keepdims=True)
    plane = PLANES[(bid % len(PLANES)).astype(int)]
    zplane = 1.0 + (bid * 0.618) % 3.0 + 0.01 * x - 0.007 * y  # a tilted plane per block; depth jumps between blocks
    is_ = {name: cls == k for k, name in enumerate(CLASSES)}
    hit = ~(is_["miss"] | is_["stray"])
    f[..., 0:3] = np.where(hit[..., None], rng.uniform(0.05, 1.0, (H, W, 3)), 1.0)
    f[..., 3] = np.where(is_["smooth"], 2.0 + 0.5 * np.sin(0.05 * x) * np.cos(0.07 * y), zplane)
    f[..., 4:7] = np.where(is_["smooth"][..., None], sm, plane)
    f[..., 7] = hit
    f[is_["miss"]] = MISS
    f[is_["stray"], 0:4] = MISS[0:4]
    f[is_["stray"], 7] = 0
    black = is_["black"]
    f[black, 0:3] = np.where((bid[black] % 2 == 0)[:, None], 0.0, [0.0, 0.5, 0.0])
    f[is_["zero_z"], 3] = 0.0
    f[hit & (rng.uniform(size=(H, W)) < 0.04), 4:7] = 0.0  # hits with a zero-length normal
    # seams: hit pixels with a miss block among their 8 neighbours cover 1/4 .. 3/4 of their samples
    mp = np.pad(is_["miss"], 1)
    near_miss = np.zeros((H, W), bool)
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            near_miss |= mp[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    seam = hit & near_miss & ~is_["zero_z"]
    cov = rng.choice([0.25, 0.5, 0.75], size=(H, W))
    for sl, miss_v in ((slice(0, 3), 1.0), (slice(3, 4), 1e5), (slice(4, 7), 0.0)):
        f[seam, sl] = cov[seam, None] * f[seam, sl] + (1 - cov[seam, None]) * miss_v
    f[seam, 7] = cov[seam]
    # accumulator: albedo x a lit gradient with noise; misses see a sky gradient; exact zeros and fireflies
    light = (0.3 + 0.7 * x / max(W - 1, 1))[..., None] * np.array([1.0, 0.8, 0.6]) + (0.5 * y / max(H - 1, 1))[..., None]
    light = light * np.maximum(0.0, 1.0 + 0.4 * rng.normal(size=(H, W, 3)))
    acc = np.ones((H, W, 4), np.float64)
    acc[..., :3] = np.where(hit[..., None], f[..., 0:3] * light, light * [0.4, 0.6, 1.2])
    acc[rng.uniform(size=(H, W)) < 0.05, :3] = 0.0
    fire = rng.uniform(size=(H, W)) < 0.01
    acc[fire, :3] = rng.uniform(16.0, 1024.0, (int(fire.sum()), 3))
    return acc.astype(np.float32), f.astype(np.float32)


def cosine_f32(n, m):
    """The cosine of two normals as k_atrous rounds it: float32 fma chains, sqrt, one product and one division (numpy
    float64 fma then rounded to float32: the same value unless a double rounding lands on a tie)."""
    n, m = np.asarray(n, np.float32), np.asarray(m, np.float32)

    def fma(a, b, c):
        return (a.astype(np.float64) * b + c).astype(np.float32)

    def dot(a, b):
        return fma(a[..., 2], b[..., 2], fma(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))

    with np.errstate(invalid="ignore", divide="ignore"):  # zero-length normals: NaN, as the kernel never asks
        return dot(n, m) / (np.sqrt(dot(n, n)) * np.sqrt(dot(m, m)))
