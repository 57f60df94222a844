#!/usr/bin/env python3
"""The GPU OpenEXR encoder on the bench scene's radiance - C2, the bunny scene at 1920x1080, depth 8, after 16
ticks (noisy) and after 1024 ticks (converged):
    kernels:  per chunk size and layer set, the three stages of fspt_exr_encode_device of the radiance (and features) from HIP
              events (rows, deflate, offsets + pack), the whole call on the host's clock, the file's size, the bytes on the bus
    host:     the path a user has without the encoder - read_radiance (and read_features), numpy's float16 conversion,
              reorder and predictor, zlib.compress per block at the default level - its time and its file's size
    forms:    the raw fallback's two forms (fspt_exr_set_form) on the rendered frame and on random bits in FLOAT, where every
              block falls back
    draw:     [tick(); read_radiance()] against [tick(); draw_exr()], ms per frame, interleaved
Every figure: --warmup untimed runs, then --reps repetitions, reported as the median with the smallest and the largest.
Prints one JSON line.
usage: python tools/exr_bench.py [--reps 7] [--frames 16] [--warmup 4] [--chunks 4096,8192,16384,32768]"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

import fspt_amd  # noqa: E402
from fspt_amd import scene as S  # noqa: E402

ALL = "alpha,albedo,normal,depth"
ORDER = [("A", 3, 0), ("B", 2, 0), ("G", 1, 0), ("N.X", 8, 0), ("N.Y", 9, 0), ("N.Z", 10, 0), ("R", 0, 0), ("Z", 7, 1), ("albedo.B", 6, 0), ("albedo.G", 5, 0), ("albedo.R", 4, 0)]
NEEDS = {"A": "alpha", "N.X": "normal", "N.Y": "normal", "N.Z": "normal", "Z": "depth", "albedo.B": "albedo", "albedo.G": "albedo", "albedo.R": "albedo"}


def note(*a):
    print(*a, file=sys.stderr, flush=True)  # (progress: the JSON line alone goes to stdout)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def host_blocks(rad, feat, layers):
    """the host's ZIP blocks of bottom-up buffers: float16 planes (Z float32), 16 scanlines, reorder, predictor, zlib level 6"""
    src = rad[::-1] if feat is None else np.concatenate([rad, feat], axis=2)[::-1]
    names = [c for c in ORDER if c[0] not in NEEDS or NEEDS[c[0]] in layers]
    planes = [np.ascontiguousarray(src[..., s]).astype(np.float32 if is_f else np.float16) for _, s, is_f in names]
    h = rad.shape[0]
    out = []
    for y0 in range(0, h, 16):
        raw = np.frombuffer(b"".join(p[y].tobytes() for y in range(y0, min(y0 + 16, h)) for p in planes), np.uint8)
        t = np.concatenate([raw[0::2], raw[1::2]])
        d = t.copy()
        d[1:] = t[1:] - t[:-1] + 128
        z = zlib.compress(d.tobytes())
        out.append(z if len(z) < raw.size else raw.tobytes())
    return out, names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--chunks", default="4096,8192,16384,32768")
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

    # the loops, interleaved - first, in a process that has not started torch yet
    forms = {"read_radiance": lambda p: p.readRadiance(), "draw_exr": lambda p: p.draw_exr(), "draw_exr_all_layers": lambda p: p.draw_exr(layers=ALL)}
    pts = {f: make() for f in forms}
    pts["draw_exr_all_layers"].features(8, 1)
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
    note("loops done")
    res = {"workload": f"C2 {W}x{H} depth {a.bounces}, ZIP", "frames_per_rep": a.frames, "readback_bytes": W * H * 16,
           "ms_per_frame": {f: spread(v) for f, v in frame_ms.items()}, "frames": {}}
    import torch

    def timed(rgba, feat, **kw):
        stages, wall = [[], [], []], []
        for k in range(a.warmup + a.reps):
            t0 = time.perf_counter()
            data = fspt_amd.exr_encode(rgba, feat, bottom_up=True, **kw)
            dt = (time.perf_counter() - t0) * 1e3
            if k >= a.warmup:
                ms, bus = fspt_amd.exr_last_ms()
                for s, v in zip(stages, ms):
                    s.append(v)
                wall.append(dt)
        return {"file_bytes": len(data), "bus_bytes": bus, "kernel_ms": {"rows": spread(stages[0]), "deflate": spread(stages[1]), "offsets_pack": spread(stages[2])},
                "encode_device_call_ms": spread(wall)}

    pt = make()
    pt.features(8, 1)
    feat = pt.readFeatures()
    dfeat = torch.from_numpy(feat).to("cuda:0")
    done = 0
    for ticks in (int(x) for x in a.ticks.split(",")):
        pt.render(ticks - done)
        done = ticks
        rad = pt.readRadiance()
        drad = torch.from_numpy(rad).to("cuda:0")
        entry = res["frames"][f"{ticks} ticks"] = {"rgb_half": {}, "all_layers_half": {}}
        for cb in chunks:
            entry["rgb_half"][str(cb)] = timed(drad, None, chunk_bytes=cb)
            entry["all_layers_half"][str(cb)] = timed(drad, dfeat, chunk_bytes=cb, layers=ALL)
        note(ticks, "ticks: chunk table done")
        entry["rgb_float_zip"] = timed(drad, None, float32=True)
        entry["rgb_half_zips"] = timed(drad, None, compression="zips")
        entry["rgb_half_none"] = timed(drad, None, compression="none")
        for name, f, layers in (("rgb_half", None, ()), ("all_layers_half", feat, ALL.split(","))):
            t = []
            for k in range(1 + min(a.reps, 3)):  # (a second or more each: one warm-up run)
                t0 = time.perf_counter()
                r = pt.readRadiance()
                ff = pt.readFeatures() if f is not None else None
                blocks, _ = host_blocks(r, ff, layers)
                if k:
                    t.append((time.perf_counter() - t0) * 1e3)
            note(ticks, "ticks: host path", name, "done")
            entry["host_" + name] = {"ms": spread(t), "blocks_bytes": sum(len(b) for b in blocks) + 16 * len(blocks)}
    # the fallback's two forms: where no block falls back (what the kept copy costs) and where every block does
    bits = torch.randint(0, 1 << 31, (H, W, 4), dtype=torch.int32, device="cuda:0").view(torch.float32)
    res["forms"] = {}
    for form in (0, 1):
        fspt_amd.exr_set_form(form)
        res["forms"][str(form)] = {"rendered_rgb_half": timed(drad, None), "random_bits_rgb_float": timed(bits, None, float32=True)}
    fspt_amd.exr_set_form(0)
    pt.close()
    print(json.dumps(res), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
