#!/usr/bin/env python3
"""What a change of the light costs, one JSON line per map size:

  (a) today's route for a map in host memory: scene.env_bins on the CPU, then Scene.update_environment(env, w, h, bins)
  (b) Scene.update_environment(env, w, h): the bins built on the GPU from the uploaded map (fspt_scene_update_environment_auto)
  (c) Scene.update_sky: generated, encoded, binned and tiled on the GPU (fspt_scene_update_sky), with the library's own split
      into sky_ms / bins_ms / tile_ms (HIP events) and its launch and read-back counts

Wall-clock milliseconds of the blocking calls, medians over --reps with the per-rep values; one unmeasured call of each route
comes first.  Nothing here is a threshold.

  python tools/sky_bench.py --reps 3
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SUN = (0.45, 0.62, 0.35)


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return (time.perf_counter() - t0) * 1e3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sizes", default="2048x1024,256x128")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from fspt_amd import Scene
    from fspt_amd import scene as S

    sc = Scene(S.bunny_scene(n=8, env_size=(64, 32)), device=args.device)
    for size in args.sizes.split(","):
        w, h = (int(v) for v in size.lower().split("x"))
        env, _, _ = S.sky(SUN, w, h, device=args.device)  # a map `in host memory` for (a) and (b): the sky (c) generates
        rows = {k: [] for k in ("a_cpu_bins", "a_update", "a_total", "b_auto", "c_sky")}
        parts = {k: [] for k in ("sky_ms", "bins_ms", "tile_ms")}
        auto_parts = {k: [] for k in ("bins_ms", "tile_ms")}
        last = None
        for rep in range(args.reps + 1):
            t_bins, bins = timed(lambda: S.env_bins(env, w, h))
            t_up, _ = timed(lambda: sc.update_environment(env, w, h, bins))
            t_auto, _ = timed(lambda: sc.update_environment(env, w, h))
            auto = sc.last_sky()
            t_sky, _ = timed(lambda: sc.update_sky(SUN, w, h))
            last = sc.last_sky()
            if rep == 0:
                continue  # (first calls: allocations of this size, code objects)
            for k, v in (("a_cpu_bins", t_bins), ("a_update", t_up), ("a_total", t_bins + t_up), ("b_auto", t_auto), ("c_sky", t_sky)):
                rows[k].append(round(v, 3))
            for k in parts:
                parts[k].append(round(last[k], 3))
            for k in auto_parts:
                auto_parts[k].append(round(auto[k], 3))
        line = dict(bench="sky", size=[w, h], reps=args.reps, n_bins=last["n_bins"], launches=last["launches"], readbacks=last["readbacks"],
                    wall_ms={k: dict(median=statistics.median(v), reps=v) for k, v in rows.items()},
                    sky_gpu_ms={k: dict(median=statistics.median(v), reps=v) for k, v in parts.items()},
                    auto_gpu_ms={k: dict(median=statistics.median(v), reps=v) for k, v in auto_parts.items()})
        print(json.dumps(line), flush=True)
    sc.close()


if __name__ == "__main__":
    main()
