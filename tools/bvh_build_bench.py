#!/usr/bin/env python3
"""tools/bvh_build_bench.py - the reference's BVH builder against the binned-SAH builder on the GPU.

    python tools/bvh_build_bench.py [--reps 3] [--configs c2,c3] [--regions 5] [--device 0]

For the BASELINE scenes c2 (bunny_scene(n=76), 69 316 triangles) and c3 (n=289, 1 002 256 triangles), prints one JSON line
per config with, for each tree ("sah": fspt_builder_build, "gpu": fspt_builder_build_gpu):
  build_s       wall time of the build call alone (the OBJ parse excluded), median of --reps;
  kernel_ms     (gpu) HIP-event time from the build's first kernel to its last, with its launches and readbacks;
  sah_cost      sum over interior nodes of SA/SA(root) + sum over leaves of n * SA/SA(root), float64 from the arrays;
  depth, nodes  of the tree;
  steps_per_ray mean traversal steps of the 960x540 camera rays (Scene.intersect);
  msamples_s    the headline render (1920x1080, 8 bounces, the wavefront pipeline) in 20-tick regions like bench.py,
                median of --regions, with the trace kernel's share from the stage timers.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

CONFIGS = {"c2": 76, "c3": 289}


def sah_cost(arrays):
    from fspt_amd import scene as S
    return S.sah_cost(arrays)  # (one place: fspt_scene_sah_cost computes the same from a scene's device boxes)


def timed_build(n, bvh, device):
    """bunny_scene(n) with the builder call timed on its own (and the GPU build's event time / launches / readbacks)"""
    from fspt_amd import _lib as L, scene as S
    lib = L.lib()
    name = "fspt_builder_build_gpu" if bvh == "gpu" else "fspt_builder_build"
    orig = getattr(lib, name)
    rec = {}

    def wrapped(b, *a):
        t0 = time.perf_counter()
        rc = orig(b, *a)
        rec["build_s"] = time.perf_counter() - t0
        if rc == 0 and bvh == "gpu":
            ms, la, rb = C.c_float(), C.c_uint32(), C.c_uint32()
            L.check(lib.fspt_builder_gpu_stats(b, C.byref(ms), C.byref(la), C.byref(rb)))
            rec.update(kernel_ms=ms.value, launches=la.value, readbacks=rb.value)
        return rc

    setattr(lib, name, wrapped)
    try:
        arrays = S.bunny_scene(n=n, env_size=(2048, 1024), bvh=bvh, device=device)
    finally:
        setattr(lib, name, orig)
    return arrays, rec


def steps_per_ray(arrays, device):
    import oracle as O
    from fspt_amd import Scene, scene as S
    cam = S.BUNNY_CAMERA
    W, H = 960, 540
    pos, d = O.camera(W, H, cam["P"], cam["I"], cam["fov_scale"], S.lens_features(cam["focal_depth"], cam["aperture"]), 77.0)
    rays = np.concatenate([pos[..., :3].reshape(-1, 3), d[..., :3].reshape(-1, 3)], 1)
    sc = Scene(arrays, device)
    try:
        _, idx, steps, _ = sc.intersect(rays)
    finally:
        sc.close()
    return float(steps.mean()), float((idx >= 0).mean())


def render_rate(arrays, regions, device):
    from fspt_amd import PathTracer, scene as S
    W, H, ticks = 1920, 1080, 20
    pt = PathTracer(arrays, W, H, device=device, num_bounces=8)
    try:
        pt.set_camera(**S.BUNNY_CAMERA)
        pt.seed(1)
        for _ in range(2):  # warm: the batch plan and the primary-form tuner settle
            pt.render(ticks)
        pt.sync()
        rates, trace = [], []
        for _ in range(regions):
            t0 = time.perf_counter()
            pt.render(ticks)
            pt.sync()
            rates.append(W * H * ticks / (time.perf_counter() - t0) / 1e6)
        pt.set_stage_timing(True)
        pt.render(ticks)
        pt.sync()
        st = pt.last_stage_ms()
        trace = st["trace"][0] / max(sum(v[0] for v in st.values()), 1e-9)
    finally:
        pt.close()
        pt.scene.close()
    return float(np.median(rates)), [round(r, 1) for r in rates], float(trace)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import fspt_amd  # noqa: F401
    for cfg in args.configs.split(","):
        n = CONFIGS[cfg]
        out = {"config": cfg, "triangles": None}
        for bvh in ("sah", "gpu"):
            recs, arrays = [], None
            for _ in range(args.reps):
                arrays, rec = timed_build(n, bvh, args.device)
                recs.append(rec)
            r = {"build_s": float(np.median([x["build_s"] for x in recs])), "build_s_all": [round(x["build_s"], 4) for x in recs]}
            if bvh == "gpu":
                r["kernel_ms"] = float(np.median([x["kernel_ms"] for x in recs]))
                r["launches"], r["readbacks"] = recs[-1]["launches"], recs[-1]["readbacks"]
            r.update(sah_cost=sah_cost(arrays), depth=arrays.depth, nodes=arrays.n_nodes)
            r["steps_per_ray"], r["hit_fraction"] = steps_per_ray(arrays, args.device)
            r["msamples_s"], r["msamples_s_regions"], r["trace_share"] = render_rate(arrays, args.regions, args.device)
            out["triangles"] = arrays.n_tris
            out[bvh] = r
            del arrays
        s, g = out["sah"], out["gpu"]
        out["ratios"] = {"build_speedup": s["build_s"] / g["build_s"], "sah_cost": g["sah_cost"] / s["sah_cost"],
                         "msamples": g["msamples_s"] / s["msamples_s"], "steps": g["steps_per_ray"] / s["steps_per_ray"]}
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
