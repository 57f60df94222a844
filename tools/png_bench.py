#!/usr/bin/env python3
"""The GPU PNG encoder on the bench scene's frame - C2, the bunny scene at 1920x1080, depth 8, drawn after 16
ticks (noisy) and after 1024 ticks (clean):
    kernels:  per chunk size, the three stages of fspt_png_encode_device of the drawn frame, from HIP events (filter, deflate,
              offsets + pack), the whole call on the host's clock, and the file's size
    draw:     [tick(); draw()] against [tick(); draw_png()], ms per frame; Pillow's PNG save of the drawn frame on this
              box's host beside them (the host path is tick + draw + that save)
    bus:      the bytes a frame brings to the host, as RGBA8 and as a file
Every figure: --warmup untimed runs, then --reps repetitions (the loop forms: of --frames frames each, interleaved), reported
as the median with the smallest and the largest.  Prints one JSON line.
usage: python tools/png_bench.py [--reps 7] [--frames 32] [--warmup 8] [--chunks 8192,16384,32768] [--channels 3]"""
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
    ap.add_argument("--frames", type=int, default=32)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--channels", type=int, default=3)
    ap.add_argument("--chunks", default="8192,16384,32768")
    ap.add_argument("--ticks", default="16,1024")
    a = ap.parse_args()
    W, H = a.width, a.height
    chunks = [int(x) for x in a.chunks.split(",")]
    arrays = S.bunny_scene(n=76, sun_deg=1.5, sun_gain=60.0)  # bench.py's C2

    def make():
        pt = fspt_amd.PathTracer(arrays, W, H, num_bounces=a.bounces)
        pt.set_camera(**S.BUNNY_CAMERA)
        pt.seed(1)
        return pt

    # the loops, interleaved - first, in a process that has not started torch yet (the device tensor below needs it)
    forms = {"draw": lambda p: p.draw(), "draw_png": lambda p: p.draw_png(channels=a.channels)}
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
    res = {"workload": f"C2 {W}x{H} depth {a.bounces}, {a.channels} channels, adaptive filter", "frames_per_rep": a.frames,
           "ms_per_frame": {f: spread(v) for f, v in frame_ms.items()}, "frames": {}}
    import torch
    pt = make()
    done = 0
    for ticks in (int(x) for x in a.ticks.split(",")):
        pt.render(ticks - done)
        done = ticks
        frame = pt.draw()
        dev = torch.from_numpy(frame).to("cuda:0")
        entry = res["frames"][f"{ticks} ticks"] = {"chunks": {}}
        for cb in chunks:
            stages, wall = [[], [], []], []
            for k in range(a.warmup + a.reps):
                t0 = time.perf_counter()
                data = fspt_amd.png_encode(dev, a.channels, "adaptive", cb, bottom_up=True)
                dt = (time.perf_counter() - t0) * 1e3
                if k >= a.warmup:
                    ms, bus = fspt_amd.png_last_ms()
                    for s, v in zip(stages, ms):
                        s.append(v)
                    wall.append(dt)
            entry["chunks"][str(cb)] = {"file_bytes": len(data), "bus_bytes": {"png": bus, "rgba8": W * H * 4},
                                        "kernel_ms": {"filter": spread(stages[0]), "deflate": spread(stages[1]), "offsets_pack": spread(stages[2])},
                                        "encode_device_call_ms": spread(wall)}
        try:
            from PIL import Image
            want = frame[::-1, :, :a.channels]
            entry["decodes_to_the_frame"] = bool(np.array_equal(np.asarray(Image.open(io.BytesIO(data))), want))
            im = Image.fromarray(want.copy())
            t = []
            for k in range(2 + a.reps):  # (half a second each: two warm-up runs)
                b = io.BytesIO()
                t0 = time.perf_counter()
                im.save(b, "PNG")
                if k >= 2:
                    t.append((time.perf_counter() - t0) * 1e3)
            entry["pillow_cpu_save_ms"] = spread(t)
            entry["pillow_file_bytes"] = len(b.getvalue())
        except ImportError:
            entry["pillow_cpu_save_ms"] = None
    pt.close()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
