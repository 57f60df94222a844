#!/usr/bin/env python3
"""The GPU JPEG encoder on the bench scene's frame - C2, the bunny scene at 1920x1080, depth 8:
    kernels:  the three stages of fspt_jpeg_encode_device of the drawn frame, from HIP events (blocks, entropy, offsets + pack)
    draw:     [tick(); draw()] against [tick(); draw_jpeg()], ms per frame
    present:  [tick(); present()] against [tick(); present_jpeg()], ms per frame
    bus:      the bytes a frame brings to the host, as RGBA8 and as a file
    pillow:   where Pillow is installed, its CPU encode of the same frame at the same settings
Every figure: --warmup untimed runs, then --reps repetitions (the loop forms: of --frames frames each, interleaved), reported
as the median with the smallest and the largest.  Prints one JSON line.
usage: python tools/jpeg_bench.py [--reps 7] [--frames 64] [--warmup 8] [--quality 85] [--444]"""
import argparse
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import fspt_amd  # noqa: E402
from fspt_amd import scene as S  # noqa: E402


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--quality", type=int, default=85)
    ap.add_argument("--444", dest="s444", action="store_true")
    a = ap.parse_args()
    W, H = a.width, a.height
    enc = dict(quality=a.quality, subsampling="444" if a.s444 else "420")
    arrays = S.bunny_scene(n=76, sun_deg=1.5, sun_gain=60.0)  # bench.py's C2

    def make():
        pt = fspt_amd.PathTracer(arrays, W, H, num_bounces=a.bounces)
        pt.set_camera(**S.BUNNY_CAMERA)
        pt.seed(1)
        return pt

    # the loops, interleaved - first, in a process that has not started torch yet (the device tensor below needs it)
    forms = {"draw": lambda p: p.draw(), "draw_jpeg": lambda p: p.draw_jpeg(**enc),
             "present": lambda p: p.present(out=out_buf), "present_jpeg": lambda p: p.present_jpeg(**enc)}
    out_buf = np.zeros((H, W, 4), np.uint8)
    pts = {f: make() for f in forms}
    frame_ms = {f: [] for f in forms}
    for rep in range(a.reps):
        for f, fn in forms.items():
            p = pts[f]
            p.clear(); p.seed(1); p.sync()
            for _ in range(a.warmup):
                p.tick(); fn(p)
            p.sync()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                p.tick(); fn(p)
            p.sync()
            frame_ms[f].append((time.perf_counter() - t0) * 1e3 / a.frames)
    for p in pts.values():
        p.close()
    # the frame: 16 ticks of C2, drawn
    pt = make()
    pt.render(16)
    frame = pt.draw()
    pt.close()
    import torch
    dev = torch.from_numpy(frame).to("cuda:0")
    stages, wall = [[], [], []], []
    for k in range(a.warmup + a.reps):
        t0 = time.perf_counter()
        data = fspt_amd.jpeg_encode(dev, bottom_up=True, **enc)
        dt = (time.perf_counter() - t0) * 1e3
        if k >= a.warmup:
            ms, bus = fspt_amd.jpeg_last_ms()
            for s, v in zip(stages, ms):
                s.append(v)
            wall.append(dt)
    res = {"workload": f"C2 {W}x{H} depth {a.bounces}, quality {a.quality}, {enc['subsampling']}, one MCU row per restart interval",
           "file_bytes": len(data), "bus_bytes": {"jpeg": bus, "rgba8": W * H * 4},
           "kernel_ms": {"blocks": spread(stages[0]), "entropy": spread(stages[1]), "offsets_pack": spread(stages[2])},
           "encode_device_call_ms": spread(wall)}
    try:
        from PIL import Image
        im = Image.fromarray(frame[::-1, :, :3].copy())
        t = []
        for k in range(a.warmup + a.reps):
            b = io.BytesIO()
            t0 = time.perf_counter()
            im.save(b, "JPEG", quality=a.quality, subsampling=0 if a.s444 else 2, optimize=False, restart_marker_rows=1)
            if k >= a.warmup:
                t.append((time.perf_counter() - t0) * 1e3)
        res["pillow_cpu_encode_ms"] = spread(t)
        res["equal_pillow_file"] = b.getvalue() == data if W % 16 == 0 and H % 16 == 0 or a.s444 else None
    except ImportError:
        res["pillow_cpu_encode_ms"] = None

    res["ms_per_frame"] = {f: spread(v) for f, v in frame_ms.items()}
    res["frames_per_rep"] = a.frames
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
