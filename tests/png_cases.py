"""tests/png_cases.py - the images and settings the PNG tests encode (tests/test_png_cpu.py, tests/test_png_gpu.py):
RGBA8 [h, w, 4] with random alpha, which matters at channels = 4 only."""
import numpy as np

from jpeg_cases import CONTENTS as JPEG_CONTENTS, image as jpeg_image

CONTENTS = JPEG_CONTENTS + ("rendered", "rows_equal", "runs")
SMALL = ((1, 1), (1, 300), (300, 1), (17, 9), (85, 3), (19, 37))
LARGE = (256, 144)  # its RGB stream: 144 * 769 = 110 736 bytes, four chunks at 32 KiB
RUNS = (1, 2, 3, 4, 257, 258, 259, 260, 516, 517, 600)
# the two code-limit cases: a size, filter 0 and one chunk that holds the whole stream
FIBONACCI = dict(w=37, h=100, channels=3, filt=0, chunk_bytes=32768)
FIBONACCI_CL = dict(w=30, h=45, channels=3, filt=0, chunk_bytes=32768)


def _fill(a, values):
    """the RGB bytes of `a` in stream order from `values`, repeated or cut"""
    h, w = a.shape[:2]
    a[..., :3] = np.resize(np.asarray(values, np.uint8), h * w * 3).reshape(h, w, 3)


def spread(counts):
    """{value: count} as a sequence in which equal values do not follow one another while another value is left: always
    the value with the most left that is not the one just placed (a tie: the lowest value)"""
    left, out, prev = dict(counts), [], None
    while left:
        v = max((k for k in left if k != prev), key=lambda k: (left[k], -k), default=prev)
        out.append(v)
        left[v] -= 1
        if not left[v]:
            del left[v]
        prev = v
    return out


def fibonacci_counts(w, h):
    """Byte values counted 1, 2, 3, 5, ... 4181 (18 of them; the end-of-block symbol is the sequence's other 1): Huffman's
    tree of the 19 symbols is a chain 18 deep.  Value 0 is the one counted 144, the h filter bytes among them; what the
    image holds beyond the sequence goes to the most frequent value, which keeps the chain."""
    out, a, b = {}, 1, 2
    for v in range(18):
        out[0 if a == 144 else v * 7 + 1] = a
        a, b = b, a + b
    out[0] -= h
    out[17 * 7 + 1] += w * h * 3 - sum(out.values())
    return out


# fibonacci_cl: dyadic counts 1 << (12 - length), so that Huffman's literal/length code has exactly CL_LENGTHS[length] codes
# of that length (Kraft sum 1 with the end-of-block symbol as the 34th code of 12 bits: 4095 bytes = 45 rows of 1 + 3 * 30).
# Values 0..83 are used, with equal lengths never next to one another in value order (symbol 16 stays out), and the 172
# unused ones behind them are two symbols 18.  The code-length code's histogram is then 1 (the distance code's length 1),
# 1, 2 (symbol 18), 3, 5, 8, 13, 21, 34: a chain 8 deep without a limit.
CL_LENGTHS = {2: 1, 3: 3, 4: 5, 8: 8, 10: 13, 11: 21, 12: 33}


def fibonacci_cl_counts(h):
    lengths = spread(CL_LENGTHS)  # the code length of byte value 0, 1, 2, ...
    k = lengths.index(4)          # value 0 is one of those counted 256: the h filter bytes and the rest in the rows
    lengths[0], lengths[k] = lengths[k], lengths[0]
    counts = {v: 1 << (12 - n) for v, n in enumerate(lengths)}
    counts[0] -= h
    return counts


def image(content, w, h, seed=0):
    if content in JPEG_CONTENTS:
        return jpeg_image(content, w, h, seed)
    rng = np.random.default_rng([seed, w, h, 16 + CONTENTS.index(content) if content in CONTENTS else 99])
    a = np.zeros((h, w, 4), np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if content == "rendered":  # smooth shading plus Gaussian noise of about 6 levels: the workload's shape
        base = np.stack([96 + 80 * np.sin(x / 37.0 + y / 91.0), 128 + 90 * np.cos(y / 53.0), 60 + (x + 2 * y) * 120.0 / max(w + 2 * h, 1)], -1)
        a[..., :3] = np.clip(np.rint(base + rng.normal(0.0, 6.0, (h, w, 3))), 0, 255)
    elif content == "rows_equal":  # every row the same noise: Up leaves zeros
        a[..., :3] = rng.integers(0, 256, (1, w, 3))
    elif content == "runs":  # with filter 0: runs of every length of RUNS, over and over, each of another value
        vals, k = [], 0
        while len(vals) < h * w * 3:
            vals += [(k * 37 + 11) & 255] * RUNS[k % len(RUNS)]
            k += 1
        _fill(a, vals)
    elif content == "fibonacci":
        _fill(a, spread(fibonacci_counts(w, h)))
    elif content == "fibonacci_cl":
        _fill(a, spread(fibonacci_cl_counts(h)))
    else:
        raise ValueError(content)
    a[..., 3] = rng.integers(0, 256, (h, w))
    return a
