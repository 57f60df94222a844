#!/usr/bin/env python3
"""tools/lights_build_bench.py - what the emitter light table costs a live-scene update, by builder.

    python tools/lights_build_bench.py --reps 7 [--sizes small,c2,c3]

One JSON line.  Per size - `small`: the bunny scene at n = 9 (976 triangles); `c2`: bench.py's c2 (69 316); `c3`: its c3
(1 002 256, tree built on the GPU) - every triangle is made emissive with Scene.update_materials (its emissive layer id
becomes its diffuse one: flat colours), so the table has about as many entries as the scene has triangles.  (A deviation from
what DESIGN 8.23's measurement first called for, ONE emissive material in c2 and in c3: that would be the cube sphere's, 4
entries fewer; the tool switches every material, so that a size's entry count is its triangle count.)  Then, with one
live tracer, medians of --reps, everything in one process, the three modes alternated rep by rep, wall clock around the
blocking calls:
  update_geometry_ms   Scene.update_geometry (the triangles breathe by 1 % about the scene's centre, so every call changes
                       every weight): refit, and with the lights on the table
  update_materials_ms  Scene.update_materials(mat) on the retained atlas: the appearance layouts, and with the lights on the table
in the modes  off (no tracer has the lights on: no table),  host (the default builder),  gpu (fspt_scene_set_light_builder),
and for the last two Scene.light_build_stats() after each call: the table's own bytes over the bus, device to host and
host to device, and its GPU ms from HIP events (the host builder's span includes the host's work between its launches).
bus_bytes adds what the update itself uploads (36 bytes per triangle of geometry, 48 of materials)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
MODES = ("off", "host", "gpu")


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def bench_size(arrays, reps, width, height):
    from fspt_amd import PathTracer, Scene
    from fspt_amd import scene as S
    mat = arrays.mat.reshape(-1, 12).copy()
    mat[:, 1] = mat[:, 0]  # emissive layer := diffuse layer
    mat = mat.reshape(-1)
    v = arrays.tri.reshape(-1, 3).astype(np.float64)
    c = (v.min(0) + v.max(0)) / 2
    tris = (arrays.tri, ((v - c) * 1.01 + c).astype(np.float32).reshape(-1))
    sc = Scene(arrays)
    pt = PathTracer(sc, width, height, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    sc.update_materials(mat, None, arrays.atlas, arrays.atlas_res, arrays.atlas_layers)  # (the first call retains the atlas)
    entries = sc.light_count()
    t = {m: {"update_geometry_ms": [], "update_materials_ms": []} for m in MODES}
    st = {m: {"update_geometry": [], "update_materials": []} for m in MODES if m != "off"}
    for r in range(reps + 1):  # (rep 0 warms every mode up: the first build of a builder allocates)
        for m in MODES[r % 3:] + MODES[:r % 3]:
            if m == "off":
                pt.set_lights("off")
            else:
                sc.set_light_builder(m)
                pt.set_lights("emitters", 0.5)
            g = timed(lambda: sc.update_geometry(tris[(r + 1) % 2]))
            sg = sc.light_build_stats() if m != "off" else None
            a = timed(lambda: sc.update_materials(mat))
            sa = sc.light_build_stats() if m != "off" else None
            if r == 0:
                continue
            t[m]["update_geometry_ms"].append(g); t[m]["update_materials_ms"].append(a)
            if m != "off":
                st[m]["update_geometry"].append(sg); st[m]["update_materials"].append(sa)
    pt.close(); sc.close()
    own = {"update_geometry": 36 * int(arrays.n_tris), "update_materials": 48 * int(arrays.n_tris)}
    res = {"n_tris": int(arrays.n_tris), "entries": int(entries), "modes": {}}
    for m in MODES:
        row = {k: float(np.median(x)) for k, x in t[m].items()}
        row["per_rep_ms"] = {k: [round(x, 4) for x in xs] for k, xs in t[m].items()}
        for k in own:
            if m == "off":
                row[k + "_bus_bytes"] = own[k]
            else:
                s = st[m][k]
                row[k + "_table"] = dict(bytes_d2h=s[-1][0], bytes_h2d=s[-1][1], gpu_ms=float(np.median([x[2] for x in s])))
                row[k + "_bus_bytes"] = own[k] + s[-1][0] + s[-1][1]
        res["modes"][m] = row
    for k in ("update_geometry_ms", "update_materials_ms"):
        res["host_over_gpu_" + k[:-3]] = res["modes"]["host"][k] / res["modes"]["gpu"][k]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--sizes", default="small,c2,c3")
    ap.add_argument("--width", type=int, default=256)
    ap.add_argument("--height", type=int, default=144)
    args = ap.parse_args(argv)
    if args.reps < 5:
        raise SystemExit("--reps must be at least 5 (the median of fewer says little)")
    import __graft_entry__ as g
    g.build()
    from fspt_amd import scene as S
    result = {"tool": "lights_build_bench", "reps": args.reps, "sizes": {}}
    for name in args.sizes.split(","):
        if name == "small":
            arrays = S.bunny_scene(n=9, env_size=(64, 32))
        elif name == "c2":
            arrays = S.bunny_scene(n=76, env_size=(64, 32))
        elif name == "c3":
            arrays = S.bunny_scene(n=289, env_size=(64, 32), bvh="gpu")
        else:
            raise SystemExit(f"unknown size {name!r} (small, c2, c3)")
        result["sizes"][name] = bench_size(arrays, args.reps, args.width, args.height)
    print(json.dumps(result))
    return 0


if __name__ == "__main__":
    sys.exit(main())
