#!/usr/bin/env python3
"""tools/camera_model_bench.py - what a camera model costs.

    python tools/camera_model_bench.py --reps 3 [--width 1920 --height 1080 --ticks 128 --bounces 8]

The C2 scene (69 316 triangles), one tracer per camera, one process, interleaved rep by rep (the first call of every tracer
is a warm-up and not timed).  One JSON line, medians of --reps:
  msamples_s           render(ticks) + sync in Msamples/s for "pinhole" (batched, today's default), "pinhole_per_tick" (the
                       two-call form undeferred, tick(): one fused tick per launch sequence - what the per-tick route is expected to
                       sit near) and the
                       four models (k_camera + the single-tick trace from the ray buffers, per tick)
  over_per_tick        a model's rate / pinhole_per_tick's;  over_batched: / pinhole's (the gap batched ray buffers would close)
  camera_ms, gb_s      the model's k_camera alone (fspt_camera_model_time: HIP events around 64 launches) and its store rate at 32
                       bytes per pixel; hbm_frac against bench.py's 8 TB/s"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure
MODELS = ("ortho", "fisheye", "equirect", "stereo")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--ticks", type=int, default=128)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--mesh-n", type=int, default=76)
    args = ap.parse_args()
    from fspt_amd import PathTracer, Scene
    from fspt_amd import _lib as L
    from fspt_amd import scene as S
    sc = Scene(S.bunny_scene(n=args.mesh_n))
    pts = {}
    for name in ("pinhole", "pinhole_per_tick") + MODELS:
        pt = PathTracer(sc, args.width, args.height, num_bounces=args.bounces)
        pt.set_camera(**S.BUNNY_CAMERA)
        if name == "pinhole_per_tick":
            pt.set_deferred(False)
        elif name != "pinhole":
            pt.set_camera_model(name)
        pts[name] = pt
    samples = args.width * args.height * args.ticks
    rate = {k: [] for k in pts}
    cam_ms = {k: [] for k in MODELS}
    for rep in range(args.reps + 1):
        for name, pt in pts.items():
            pt.clear(); pt.sync()
            t0 = time.perf_counter()
            if name == "pinhole_per_tick":
                for _ in range(args.ticks):
                    pt.tick()
            else:
                pt.render(args.ticks)
            pt.sync()
            dt = time.perf_counter() - t0
            if rep:
                rate[name].append(samples / dt / 1e6)
        for name in MODELS:
            ms = C.c_float()
            L.check(L.lib().fspt_camera_model_time(pts[name]._t, C.byref(pts[name]._camera_params()), 64, C.byref(ms)))
            if rep:
                cam_ms[name].append(ms.value)
    med = lambda x: float(np.median(x))
    out = {"width": args.width, "height": args.height, "ticks": args.ticks, "bounces": args.bounces, "reps": args.reps,
           "triangles": int(sc.arrays.n_tris),
           "msamples_s": {k: round(med(v), 1) for k, v in rate.items()},
           "msamples_s_all": {k: [round(x, 1) for x in v] for k, v in rate.items()}}
    out["over_per_tick"] = {k: round(med(rate[k]) / med(rate["pinhole_per_tick"]), 3) for k in MODELS}
    out["over_batched"] = {k: round(med(rate[k]) / med(rate["pinhole"]), 3) for k in MODELS + ("pinhole_per_tick",)}
    gb = args.width * args.height * 32 / 1e9
    out["camera_ms"] = {k: round(med(v), 5) for k, v in cam_ms.items()}
    out["gb_s"] = {k: round(gb / (med(v) * 1e-3), 1) for k, v in cam_ms.items()}
    out["hbm_frac"] = {k: round(gb / (med(v) * 1e-3) / HBM_PEAK_GBS, 3) for k, v in cam_ms.items()}
    print(json.dumps(out))
    for pt in pts.values():
        pt.close()
    sc.close()


if __name__ == "__main__":
    main()
