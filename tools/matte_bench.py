"""tools/matte_bench.py - the measurements of DESIGN 8.25 (ID mattes), one JSON line each.

  pass   fspt_mattes at 1920 x 1080 on the bench scene, 8 samples, with one kind and with two, against fspt_features of the
         same samples and seed (the same rays; unchanged code): the three are timed interleaved, --reps times each, host
         clock around call + fspt_sync; medians, and the spread (max - min) of fspt_features' own repetitions as the margin
  file   draw_exr with both matte layers (only the file crosses the bus) against read_mattes x 2 + readRadiance and the
         host's numpy + zlib making a file of the same channels: milliseconds and bytes on the bus

    python tools/matte_bench.py [--width 1920 --height 1080 --samples 8 --reps 9 --mesh-n 76]
"""
import argparse
import json
import os
import statistics
import struct
import sys
import time
import zlib

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fspt_amd  # noqa: E402
from fspt_amd import PathTracer, scene as S  # noqa: E402


def timed(pt, fn):
    pt.sync()
    t0 = time.perf_counter()
    fn()
    pt.sync()
    return (time.perf_counter() - t0) * 1e3


def host_file(rgba, ranks):
    """what a host without the encoder would do with the buffers it read: HALF R G B, FLOAT matte channels, ZIP blocks of
    16 scanlines (even / odd bytes, deltas) through zlib - the layout of the file, not its exact bytes"""
    h, w = rgba.shape[:2]
    top = rgba[::-1]
    planes = [top[..., c].astype(np.float16).view(np.uint16) for c in (2, 1, 0)]
    for r in ranks:
        planes += [r[::-1][..., c].view(np.uint32) for c in range(12)]
    out = bytearray()
    for y0 in range(0, h, 16):
        raw = b"".join(p[y].tobytes() for y in range(y0, min(y0 + 16, h)) for p in planes)
        a = np.frombuffer(raw, np.uint8)
        t = np.concatenate([a[0::2], a[1::2]]).astype(np.int16)
        t[1:] = (t[1:] - t[:-1] + 128) & 255
        z = zlib.compress(t.astype(np.uint8).tobytes(), 6)
        out += struct.pack("<ii", y0, len(z)) + z
    return bytes(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--mesh-n", type=int, default=76)
    a = ap.parse_args()
    arrays = S.bunny_scene(n=a.mesh_n, keep_order=True)
    W, H, n = a.width, a.height, a.samples
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.seed(1)
    pt.render(4)
    sc = pt.scene

    def kinds(two):
        sc.set_default_mattes()
        if not two:
            sc.set_matte("material", None, None)

    runs = {"features": [], "mattes_1": [], "mattes_2": []}
    for warm in (True, False):
        for _ in range(1 if warm else a.reps):
            f = timed(pt, lambda: pt.features(n, 1))
            kinds(False)
            m1 = timed(pt, lambda: pt.mattes(n, 1))
            kinds(True)
            m2 = timed(pt, lambda: pt.mattes(n, 1))
            if not warm:
                runs["features"].append(f); runs["mattes_1"].append(m1); runs["mattes_2"].append(m2)
    med = {k: statistics.median(v) for k, v in runs.items()}
    print(json.dumps({"bench": "pass", "width": W, "height": H, "samples": n, "triangles": int(arrays.n_tris), "reps": a.reps,
                      "median_ms": med, "features_spread_ms": max(runs["features"]) - min(runs["features"]),
                      "min_ms": {k: min(v) for k, v in runs.items()}, "max_ms": {k: max(v) for k, v in runs.items()},
                      "lost": [pt.mattes_lost(0), pt.mattes_lost(1)]}))

    layers = ("crypto_object", "crypto_material")
    gpu, host, size = [], [], 0
    for warm in (True, False):
        for _ in range(1 if warm else a.reps):
            t0 = time.perf_counter()
            data = pt.draw_exr(layers=layers)
            t1 = time.perf_counter()
            rgba, ranks = pt.readRadiance(), [pt.read_mattes(k, raw=True) for k in (0, 1)]
            t2 = time.perf_counter()
            ref = host_file(rgba, ranks)
            t3 = time.perf_counter()
            if not warm:
                gpu.append((t1 - t0) * 1e3); host.append(((t2 - t1) * 1e3, (t3 - t2) * 1e3))
            size = len(data)
    print(json.dumps({"bench": "file", "width": W, "height": H, "draw_exr_ms": statistics.median(gpu), "draw_exr_bus_bytes": size + 8, "file_bytes": size,
                      "host_read_ms": statistics.median(x for x, _ in host), "host_encode_ms": statistics.median(y for _, y in host),
                      "host_bus_bytes": W * H * (16 + 48 + 48), "host_file_bytes": len(ref)}))
    pt.close()


if __name__ == "__main__":
    main()
