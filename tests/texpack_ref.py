"""The texture packer's arithmetic contract restated in numpy, and the cases both test files share.

Written from the contract, not from scene.resample_image: float32 throughout, every operation rounded on its own, the two
decode tables taken from fspt_texture_decode_tables.  pack() is the whole raw atlas of a description in that statement."""
import ctypes as C
import math

import numpy as np

from fspt_amd import _lib as L
from fspt_amd import scene as S

F = np.float32
_TABLES = None


def tables():
    global _TABLES
    if _TABLES is None:
        _TABLES = S.texture_decode_tables()
    return _TABLES


def resample(rgba, res, corrected=False, swizzle=(0, 1, 2, 3)):
    """One layer: rgba uint8 [h, w, 4] (row 0 = top) -> uint8 [res, res, 4] (row 0 = bottom)."""
    rgba = np.asarray(rgba, np.uint8)
    h, w = rgba.shape[:2]
    lin, srgb = tables()
    px = (np.arange(res).astype(F) + F(0.5)) / F(res)
    u = px * F(w) - F(0.5)
    v = (F(1.0) - px) * F(h) - F(0.5)
    fu, fv = np.floor(u), np.floor(v)
    a, b = (u - fu).astype(F), (v - fv).astype(F)
    i0 = np.mod(fu.astype(np.int64), w)
    i1 = np.mod(fu.astype(np.int64) + 1, w)
    j0 = np.clip(fv.astype(np.int64), 0, h - 1)
    j1 = np.clip(fv.astype(np.int64) + 1, 0, h - 1)
    dec = np.empty((h, w, 4), F)
    rgb_tab = srgb if corrected else lin
    dec[..., :3] = rgb_tab[rgba[..., :3]]
    dec[..., 3] = lin[rgba[..., 3]]
    A, nA = a[None, :, None], (F(1.0) - a)[None, :, None]
    B, nB = b[:, None, None], (F(1.0) - b)[:, None, None]
    top = dec[j0][:, i0] * nA + dec[j0][:, i1] * A
    bot = dec[j1][:, i0] * nA + dec[j1][:, i1] * A
    c = top * nB + bot * B
    assert c.dtype == F
    c = c[..., list(swizzle)]
    q = np.floor(c[..., :3] * c[..., 3:4] * F(255.0) + F(0.5))
    assert q.dtype == F
    out = np.empty((res, res, 4), np.uint8)
    out[..., :3] = np.clip(q, 0, 255).astype(np.uint8)
    out[..., 3] = 255
    return out


def color_texel(color):
    return [int(math.floor(min(max(float(c), 0.0), 1.0) * 255.0 + 0.5)) for c in color[:3]] + [255]


def pack(desc):
    """The raw atlas of a pack_desc()-style description: uint8 [layers * res * res * 4]."""
    res = int(desc["res"])
    out = np.zeros((len(desc["layers"]), res, res, 4), np.uint8)
    for l, y in enumerate(desc["layers"]):
        if y["kind"] == "color":
            out[l] = np.array(color_texel(y["color"]), np.uint8)
        elif y["kind"] == "pixels":
            out[l] = np.asarray(desc["images"][y["image"]], np.uint8)
        else:
            out[l] = resample(desc["images"][y["image"]], res, y.get("corrected", False), y.get("swizzle") or (0, 1, 2, 3))
    return out.reshape(-1)


# ---- cases ----
SOURCE_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (3, 5), (16, 16), (33, 17), (64, 48), (300, 200)]  # (w, h)
RESOLUTIONS = [1, 2, 3, 5, 8, 9, 16, 33]
SWIZZLES = [(0, 1, 2, 3), (0, 2, 1, 3), (3, 2, 1, 0), (1, 1, 1, 1)]
CPU_SHAPES = [((1, 1), 4), ((3, 5), 8), ((7, 2), 9), ((16, 16), 16), ((33, 17), 5), ((64, 48), 33)]  # ((w, h), res)


def source(w, h, seed=0):
    """A w x h RGBA8 image with alpha below 255, bytes 0 and 255, and a gradient whose premultiplied products land on .5
    ties (byte pairs (c, alpha) with c * alpha / 255 = k + 0.5 exactly, e.g. (51, 5) -> 1.0 / 255 ... and (255, 128), (85, 3))."""
    rng = np.random.default_rng(1000 * w + h + seed)
    im = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    im[..., 0] = (xx * 255 // max(w - 1, 1)).astype(np.uint8)            # a gradient 0 .. 255
    ties = np.array([(255, 128), (85, 3), (51, 5), (17, 15), (0, 255), (255, 0), (255, 255), (1, 255)], np.uint8)
    k = (xx + 3 * yy) % (2 * len(ties))
    use = k < len(ties)
    im[..., 1] = np.where(use, ties[k % len(ties), 0], im[..., 1])
    im[..., 3] = np.where(use, ties[k % len(ties), 1], im[..., 3])
    im.reshape(-1, 4)[0] = (0, 255, 0, 255)
    im.reshape(-1, 4)[-1] = (255, 0, 255, 0 if w * h > 1 else 255)
    return im


def image_layer(image, corrected=False, swizzle=(0, 1, 2, 3)):
    return {"kind": "image", "image": image, "corrected": corrected, "swizzle": tuple(swizzle)}


# ---- a good description and the ways to spoil its ctypes form (fspt_texture_pack): every FSPT_E_INVALID of a description ----
def good_desc(res=4):
    return {"res": res, "images": [source(3, 5), np.zeros((res, res, 4), np.uint8)],
            "layers": [{"kind": "color", "color": [0.1, 0.2, 0.3]}, image_layer(0, True, (0, 2, 1, 3)), {"kind": "pixels", "image": 1}]}


def _set(path, value):
    def f(p):
        obj = p
        for k in path[:-1]:
            obj = obj[k] if isinstance(k, int) else getattr(obj, k)
        if isinstance(path[-1], int):
            obj[path[-1]] = value
        else:
            setattr(obj, path[-1], value)
    return f


INVALID = {
    "null_layers": _set(("layers",), C.POINTER(L.TextureLayer)()),
    "null_images": _set(("images",), C.POINTER(L.TextureImage)()),
    "null_rgba": _set(("images", 0, "rgba"), None),
    "res_0": _set(("res",), 0),
    "res_16385": _set(("res",), 16385),
    "w_0": _set(("images", 0, "w"), 0),
    "h_0": _set(("images", 0, "h"), 0),
    "w_16385": _set(("images", 0, "w"), 16385),
    "h_16385": _set(("images", 0, "h"), 16385),
    "no_layers": _set(("n_layers",), 0),
    "image_index": _set(("layers", 1, "image"), 2),
    "pixels_image_index": _set(("layers", 2, "image"), 7),
    "swizzle_4": _set(("layers", 1, "swizzle", 2), 4),
    "kind_3": _set(("layers", 1, "kind"), 3),
    "kind_negative": _set(("layers", 0, "kind"), -1),
    "colour_nan": _set(("layers", 0, "color", 1), float("nan")),
    "colour_inf": _set(("layers", 0, "color", 2), float("inf")),
    "pixels_not_res": _set(("layers", 2, "image"), 0),
}
