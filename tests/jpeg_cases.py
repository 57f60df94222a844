"""tests/jpeg_cases.py - the images the JPEG tests encode (tests/test_jpeg_cpu.py, tests/test_jpeg_gpu.py): RGBA8 [h, w, 4]
with random alpha, which must not matter."""
import numpy as np

CONTENTS = ("noise", "gradient", "saturated", "constant", "checkerboard")


def image(content, w, h, seed=0):
    rng = np.random.default_rng([seed, w, h, CONTENTS.index(content)])
    a = np.zeros((h, w, 4), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if content == "noise":
        a[..., :3] = rng.integers(0, 256, (h, w, 3))
    elif content == "gradient":
        a[..., 0] = (x * 255) // max(w - 1, 1)
        a[..., 1] = (y * 255) // max(h - 1, 1)
        a[..., 2] = ((x + y) * 255) // max(w + h - 2, 1)
    elif content == "saturated":  # every channel 0 or 255, in patches and single texels
        a[..., :3] = rng.integers(0, 2, (h, w, 3)) * 255
        a[: h // 2, : w // 2, :3] = 255
        a[h // 2:, w // 2:, :3] = 0
    elif content == "constant":
        a[..., :3] = (201, 17, 96)
    else:  # a one-pixel checkerboard: energy in the highest frequency alone, long zero runs in front of it (ZRL)
        a[..., :3] = (((x + y) & 1) * 255)[..., None]
    a[..., 3] = rng.integers(0, 256, (h, w))
    return a
