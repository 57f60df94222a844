#!/usr/bin/env python3
"""tools/mesh_bench.py - Scene.update_vertices against the two ways to move the vertices of the same mesh without it
(DESIGN 8.24).

    python tools/mesh_bench.py --reps 7 [--grids 23,188,709] [--normals flat,smooth]

Per grid (n x n vertices, 2 (n - 1)^2 triangles: 968, 69 938, 1 002 528; the tree built on the GPU) and normals mode one
JSON line.  A frame displaces every vertex along z by a travelling wave.  Timed in one process, interleaved rep by rep,
the first call of every path not timed; per column the median and the values:
  update_vertices_s        Scene.update_vertices, host form: 12 bytes per vertex up, the derive kernels, the refit
  update_vertices_device_s the same from a torch tensor on the device: nothing crosses the bus
  derive_ms, pass_ms, refit_ms, launches   its parts on the GPU (Scene.last_mesh); pass_ms = k_mesh_faces,
                           k_mesh_vertex_normals, k_mesh_smooth_frames
  builder_host_s (builder_s + host_update_s)   the frame written as OBJ text, parsed and derived by the native builder
                           (build_scene(geometry_only=True)), put in leaf order, then the host form of update_geometry
                           (144 bytes per triangle up, the refit)
  numpy_host_s (numpy_s + host_update_s)       the same arrays from tests/mesh_ref.py's numpy float64 restatement
  bus_bytes                what crosses the bus per frame: update_vertices | update_geometry
  derive_bytes             what the derive kernels must move, counted from the shapes (T triangles, V vertices, A = 3 T
                           incident corners):
                             flat    T x (12 idx + 36 pos + 24 cst + 4 face + 36 tri + 108 norm)               = 220 T
                             smooth  faces   T x (12 + 36 + 4 + 36 tri + 24 fnorm)                              = 112 T
                                     vertex  V x (8 offsets + 24 vnorm) + A x (4 face id + 24 fnorm)            = 32 V + 84 T
                                     frames  T x (12 + 4 + 36 tri + 24 cst + 72 vnorm + 108 norm)               = 256 T
  derive_gb_s, hbm_frac    derive_bytes over derive_ms; against bench.py's 8 TB/s
  skin_ms, skin_gb_s       the yardstick: k_skin_transform (one joint per corner slot of 16, rest normals, no morphs: 360
                           bytes per triangle) on the same T in the same run"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure
SKIN_BYTES_PER_TRI = 24 + 48 + 144 + 144


def grid(n):
    """(positions [n n, 3] float32, faces [T, 3], OBJ tail: the vt and f lines)"""
    ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    pos = np.stack([xs.reshape(-1) / (n - 1) * 2.0 - 1.0, np.zeros(n * n), ys.reshape(-1) / (n - 1) * 2.0 - 1.0], axis=1).astype(np.float32)
    a = (ys[:-1, :-1] * n + xs[:-1, :-1]).reshape(-1)
    faces = np.concatenate([np.stack([a, a + n + 1, a + 1], 1), np.stack([a, a + n, a + n + 1], 1)])
    vt = "".join("vt %r %r\n" % (float(x) / (n - 1) * 0.9 + 0.05, float(y) / (n - 1) * 0.9 + 0.05) for y in range(n) for x in range(n))
    f = "".join("f %d/%d %d/%d %d/%d\n" % (i + 1, i + 1, j + 1, j + 1, k + 1, k + 1) for i, j, k in faces)
    return pos, faces, vt + f


def obj_text(pos, tail):
    return "".join("v %r %r %r\n" % (float(x), float(y), float(z)) for x, y, z in pos) + tail


def frame(pos, k):
    p = pos.copy()
    p[:, 1] = np.float32(0.15) * np.sin(np.float32(5.0) * pos[:, 0] + np.float32(0.4 * k)) * np.cos(np.float32(3.0) * pos[:, 2])
    return p


def derive_bytes(T, V, smooth):
    return 112 * T + (32 * V + 84 * T) + 256 * T if smooth else 220 * T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--grids", default="23,188,709")
    ap.add_argument("--normals", default="flat,smooth")
    ap.add_argument("--skip-host-above", type=int, default=2_000_000, help="triangles above which the builder / numpy columns are left out")
    args = ap.parse_args()
    import torch
    import mesh_ref as R
    from fspt_amd import Scene
    from fspt_amd import scene as S
    med = lambda x: float(np.median(x))
    for n in (int(x) for x in args.grids.split(",")):
        pos0, faces, tail = grid(n)
        for normals in args.normals.split(","):
            prop = {"path": "g.obj", "normals": normals, "diffuse": [0.7, 0.6, 0.5], "emittance": [0, 0, 0]}
            env, w, h = S.synthetic_env(64, 32)
            arrays = S.build_scene([prop], {"g.obj": obj_text(frame(pos0, 0), tail)}, env=env, env_w=w, env_h=h, bvh="gpu", keep_order=True, keep_mesh=True)
            T, V, m = arrays.n_tris, arrays.meta["n_vertices"], arrays.meta
            M, Dv, Hb = Scene(arrays), Scene(arrays), Scene(arrays)
            M.set_mesh(); Dv.set_mesh()
            joints = np.zeros((T, 3, 4), np.uint16); joints[..., 0] = (np.arange(T * 3) % 16).reshape(T, 3)
            weights = np.zeros((T, 3, 4), np.float32); weights[..., 0] = 1.0
            K = Scene(arrays); K.set_skin(joints, weights, n_joints=16)
            xf = np.tile(np.eye(3, 4, dtype=np.float32).reshape(12), (16, 1))
            host = T <= args.skip_host_above
            tv, td, tk, tp, tr, tb, tn, th, ts, nl = [], [], [], [], [], [], [], [], [], 0
            for k in range(args.reps + 1):
                p = frame(pos0, k + 1)
                t0 = time.perf_counter(); M.update_vertices(p); a = time.perf_counter() - t0
                ms = M.last_mesh
                d_p = torch.from_numpy(p).to("cuda:0"); torch.cuda.synchronize()
                t0 = time.perf_counter(); Dv.update_vertices(d_p); b = time.perf_counter() - t0
                K.update_skin(xf)
                if k:
                    tv.append(a); td.append(b); tk.append(ms["derive_ms"]); tp.append(ms["pass_ms"]); tr.append(ms["refit_ms"]); nl = ms["launches"]
                    ts.append(K.last_skin["skin_ms"])
                if not host:
                    continue
                t0 = time.perf_counter()
                g = S.build_scene([prop], {"g.obj": obj_text(p, tail)}, geometry_only=True)
                tri, norm = S.geometry_in_leaf_order(arrays, g.tri, g.norm)
                c = time.perf_counter() - t0
                t0 = time.perf_counter(); Hb.update_geometry(tri, norm); d = time.perf_counter() - t0
                t0 = time.perf_counter(); R.mesh_ref(m["tri_vertex"], m["tri_uv64"], p, m["tri_smooth"], m["tri_order"]); e = time.perf_counter() - t0
                if k:
                    tb.append(c); th.append(d); tn.append(e)
            nbytes = derive_bytes(T, V, normals == "smooth")
            gbs = nbytes / (med(tk) * 1e-3) / 1e9
            sgbs = T * SKIN_BYTES_PER_TRI / (med(ts) * 1e-3) / 1e9
            line = dict(grid=n, triangles=T, vertices=V, normals=normals, reps=args.reps,
                        update_vertices_s=med(tv), update_vertices_s_all=tv, update_vertices_device_s=med(td), update_vertices_device_s_all=td,
                        derive_ms=med(tk), derive_ms_all=tk, pass_ms=[med([x[i] for x in tp]) for i in range(3)], refit_ms=med(tr), launches=nl,
                        bus_bytes=[V * 12, T * 144], mesh_bytes=M.last_mesh["bytes"], derive_bytes=nbytes, derive_gb_s=gbs, hbm_frac=gbs / HBM_PEAK_GBS,
                        skin_ms=med(ts), skin_gb_s=sgbs, derive_over_skin=gbs / sgbs)
            if host:
                line.update(builder_s=med(tb), numpy_s=med(tn), host_update_s=med(th), builder_host_s=med(np.add(tb, th)), numpy_host_s=med(np.add(tn, th)),
                            builder_over_mesh=med(np.add(tb, th)) / med(tv), numpy_over_mesh=med(np.add(tn, th)) / med(tv))
            print(json.dumps(line), flush=True)
            for sc in (M, Dv, Hb, K):
                sc.close()


if __name__ == "__main__":
    main()
