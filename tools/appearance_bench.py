#!/usr/bin/env python3
"""tools/appearance_bench.py - fspt_scene_update_materials / _environment against re-creating the scene.

    python tools/appearance_bench.py --reps 3 [--scenes textured,e3]

One JSON line.  Per scene - `textured`: bench.py's image-mapped scene (69 316 triangles, 2048^2 atlas); `e3`: the flat-colour
emitter scene of tests/lights_ref.py - medians of --reps, everything timed in one process, interleaved rep by rep, wall
clock around the blocking calls:
  recreate_s      closing and re-creating Scene + PathTracer + prepare() from the arrays through the unchanged entry points:
                  the only way to change a look without the feature
  materials_s     Scene.update_materials(mat, uv, atlas, ...) on a scene with a live, prepared tracer
  materials_kept_s  Scene.update_materials(mat, uv) - the retained atlas is laid out again, nothing of it is uploaded
  environment_s   Scene.update_environment(env, w, h, bins)
and for the three updates Scene.last_appearance(): kernel ms first to last (HIP events; read-back and host classification
between them), launches, bytes uploaded, raw-atlas bytes retained.  The update alternates between the scene's own
appearance and a changed one (other layer ids on a tenth of the triangles, an atlas with one layer inverted, the
environment mirrored), so every timed call changes something."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def variant(a):
    import dataclasses
    mat = a.mat.reshape(-1, 12).copy()
    k = max(a.n_tris // 10, 1)
    mat[:k, 0], mat[:k, 3] = mat[:k, 3].copy(), mat[:k, 0].copy()  # diffuse <-> mr layer ids on a tenth of the triangles
    atlas = a.atlas.copy().reshape(a.atlas_layers, -1)
    atlas[-1] = 255 - atlas[-1]
    env = None if a.env is None else a.env.reshape(a.env_h, a.env_w, 4)[:, ::-1].copy().reshape(-1)
    from fspt_amd import scene as S
    bins = a.bins if env is None else S.env_bins(env, a.env_w, a.env_h)
    return dataclasses.replace(a, mat=mat.reshape(-1), atlas=atlas.reshape(-1), env=env, bins=bins)


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bench_scene(arrays, reps, width, height):
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S
    looks = (arrays, variant(arrays))
    live = Scene(arrays)
    pt = PathTracer(live, width, height, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.prepare()
    live.update_materials(arrays.mat, arrays.uv, arrays.atlas, arrays.atlas_res, arrays.atlas_layers)  # (first call: allocates the retained atlas)
    out = {k: [] for k in ("recreate_s", "materials_s", "materials_kept_s", "environment_s")}
    last = {}
    for r in range(reps):
        a = looks[(r + 1) % 2]

        def recreate():
            sc = Scene(a)
            p2 = PathTracer(sc, width, height, num_bounces=4)
            p2.set_camera(**S.BUNNY_CAMERA)
            p2.prepare()
            p2.sync()
            p2.close(); sc.close()

        out["materials_s"].append(timed(lambda: live.update_materials(a.mat, a.uv, a.atlas, a.atlas_res, a.atlas_layers)))
        last.setdefault("materials", []).append(live.last_appearance())
        b = looks[r % 2]
        out["materials_kept_s"].append(timed(lambda: live.update_materials(b.mat, b.uv)))
        last.setdefault("materials_kept", []).append(live.last_appearance())
        out["environment_s"].append(timed(lambda: live.update_environment(a.env, a.env_w, a.env_h, a.bins)))
        last.setdefault("environment", []).append(live.last_appearance())
        # last in the rep: what the driver defers of freeing a tracer's path state is paid by the next large allocation -
        # which is the next rep's re-creation, the path that caused it
        out["recreate_s"].append(timed(recreate))
    pt.close(); live.close()
    res = {k: float(np.median(v)) for k, v in out.items()}
    res["per_rep_s"] = {k: [round(x, 6) for x in v] for k, v in out.items()}
    for k, v in last.items():
        res[k] = dict(kernel_ms=float(np.median([x["ms"] for x in v])), launches=v[-1]["launches"], uploaded=v[-1]["uploaded"],
                      retained=v[-1]["retained"])
    res.update(n_tris=int(arrays.n_tris), atlas=f"{arrays.atlas_res}^2 x {arrays.atlas_layers}", env=f"{arrays.env_w} x {arrays.env_h}",
               upload_bound_bytes_per_tri=72)
    for k in ("materials_s", "materials_kept_s", "environment_s"):
        res["recreate_over_" + k[:-2]] = res["recreate_s"] / res[k] if res[k] > 0 else None
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--scenes", default="textured,e3")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    args = ap.parse_args(argv)
    import __graft_entry__ as g
    g.build()
    from fspt_amd import scene as S
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    result = {"tool": "appearance_bench", "reps": args.reps, "resolution": [args.width, args.height], "scenes": {}}
    for name in args.scenes.split(","):
        if name == "textured":
            arrays = S.bunny_scene_textured()
        elif name == "e3":
            import lights_ref as LR
            arrays = LR.scene_e3()
        else:
            raise SystemExit(f"unknown scene {name!r} (textured, e3)")
        result["scenes"][name] = bench_scene(arrays, max(args.reps, 1), args.width, args.height)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
