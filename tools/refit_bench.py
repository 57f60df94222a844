#!/usr/bin/env python3
"""tools/refit_bench.py - fspt_scene_update_geometry and fspt_scene_rebuild_geometry against rebuilding the scene.

    python tools/refit_bench.py --reps 3 [--configs c2,c3]

Per config (c2: 69 316 triangles, c3: 1 002 256) and move - a rigid rotation of the whole scene by 2 degrees, a sine-wave
deformation with an amplitude of 1 % and of 10 % of the scene's size - one JSON line with, medians of --reps, timed in one
process, interleaved rep by rep:
  update_host_s / update_device_s   the update call (numpy arrays: upload + refit; a torch tensor on the device: refit)
  update_kernel_ms, launches        its kernels, first to last (HIP events; the finite check's 4-byte readback lies between)
  bytes, gb_s, hbm_frac             what the kernels move (below) over update_kernel_ms, against bench.py's 8 TB/s
  rebuild_s, rebuild_parts_s        the only way to do the same without the feature: fspt_builder_build_gpu on the moved
                                    triangles + fspt_scene_create + a new target + prepare() (OBJ parsing NOT counted:
                                    the builder is fed before the clock starts)
  inplace_host_s / inplace_device_s  Scene.rebuild_geometry on a second scene with a live, prepared target: a new
                                    tree in place from numpy arrays / from a torch tensor on the device; inplace_split =
                                    the device form's fspt_scene_last_rebuild_ms (build_ms, install_ms, host_ms, launches,
                                    readbacks); rebuild_over_inplace_device = rebuild_s / inplace_device_s
  sah_before / sah_refit / sah_inplace / sah_fresh   Scene.sah_cost() of the base tree, the refitted one, the one rebuilt in
                                    place, a tree built on the moved triangles by the rebuild path
  msamples_refit / msamples_inplace / msamples_fresh   1920 x 1080, 8 bounces, 20-tick regions, on those three trees
Bytes per triangle, counted from the kernels: check 36 x 4 read; records 36 x 4 read + per leaf slot 9 x 4 (leaf record)
+ 36 x 4 (hit record) written; leaf boxes 9 x 4 read + 24 written per leaf; levels 48 read + 24 written per interior node;
two-level nodes 2 x 64 read + 128 written per interior node."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": 76, "c3": 289}
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure


def rotate(tri, norm, deg):
    th = np.radians(deg)
    M = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    v = tri.reshape(-1, 3).astype(np.float64)
    c = (v.min(0) + v.max(0)) / 2
    return (((v - c) @ M.T) + c).astype(np.float32).reshape(-1), (norm.reshape(-1, 3).astype(np.float64) @ M.T).astype(np.float32).reshape(-1)


def sine(tri, amp):
    v = tri.reshape(-1, 3).astype(np.float64).copy()
    size = float((v.max(0) - v.min(0)).max())
    v[:, 1] += amp * size * np.sin(3 * np.pi * v[:, 0] / size)
    return v.astype(np.float32).reshape(-1)


def obj_of(tri):
    """an OBJ text of the moved triangles (one `v` per corner), so that a builder can be fed them"""
    v = tri.reshape(-1, 3).astype(np.float64)
    lines = ["v %.9g %.9g %.9g" % tuple(p) for p in v]
    lines += ["f %d %d %d" % (3 * i + 1, 3 * i + 2, 3 * i + 3) for i in range(v.shape[0] // 3)]
    return "\n".join(lines) + "\n"


def rebuild(base, text, device, W, H):
    """the rebuild path on the moved triangles; returns (seconds without parsing, Scene, PathTracer, (build, get + permute,
    scene create, target + prepare) seconds)"""
    import dataclasses
    from fspt_amd import PathTracer, Scene, _lib as L
    lib = L.lib()
    b = C.c_void_p()
    L.check(lib.fspt_builder_create(C.byref(b)))
    try:
        pd = L.PropDesc(); pd.scale = 1.0
        L.check(lib.fspt_builder_add_obj(b, text, len(text), C.byref(pd)))
        t0 = time.perf_counter()
        L.check(lib.fspt_builder_build_gpu(b, base.leaf_size, device))
        t1 = time.perf_counter()
        nn, nt, dp = C.c_uint32(), C.c_uint32(), C.c_uint32()
        L.check(lib.fspt_builder_counts(b, C.byref(nn), C.byref(nt), C.byref(dp)))
        bvh = np.zeros(nn.value * 9, np.float32); t2 = np.zeros(nt.value * 9, np.float32)
        order = np.zeros(nt.value, np.uint32)
        L.check(lib.fspt_builder_get(b, L.fptr(bvh), L.fptr(t2), None, None, None))
        L.check(lib.fspt_builder_tri_order(b, L.u32ptr(order)))
        # materials / normals / uvs follow the triangles into the new leaf order (the base's arrays, permuted)
        arr = dataclasses.replace(base, bvh=bvh, tri=t2, mat=np.ascontiguousarray(base.mat.reshape(-1, 12)[order]).reshape(-1),
                                  norm=np.ascontiguousarray(base.norm.reshape(-1, 27)[order]).reshape(-1),
                                  uv=np.ascontiguousarray(base.uv.reshape(-1, 6)[order]).reshape(-1), depth=dp.value)
        t2_ = time.perf_counter()
        sc = Scene(arr, device)
        t3 = time.perf_counter()
        pt = PathTracer(sc, W, H, device=device, num_bounces=8)
        pt.prepare()
        pt.sync()
        t4 = time.perf_counter()
        return t4 - t0, sc, pt, (t1 - t0, t2_ - t1, t3 - t2_, t4 - t3)
    finally:
        lib.fspt_builder_destroy(b)


def rate(pt, regions=3, ticks=20):
    from fspt_amd import scene as S
    W, H = pt.resolution
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.seed(1)
    for _ in range(2):
        pt.render(ticks)
    pt.sync()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        pt.render(ticks)
        pt.sync()
        out.append(W * H * ticks / (time.perf_counter() - t0) / 1e6)
    return float(np.median(out))


def moved_bytes(arrays, with_norm, quads):
    w = arrays.bvh.reshape(-1, 9)[:, :3].view(np.int32)
    leaves = int((w[:, 2] > -1).sum()); interior = arrays.n_nodes - leaves
    T, slots = arrays.n_tris, leaves * arrays.leaf_size
    k = 36 if with_norm else 9
    b = T * k * 4 + slots * (k + 9 + k) * 4 + T * 36 + leaves * 24 + interior * 72
    if quads:
        b += interior * 256
    return b


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--no-rate", action="store_true", help="skip the render-rate comparison")
    args = ap.parse_args()
    import torch
    from fspt_amd import PathTracer, Scene, scene as S
    W, H = 1920, 1080
    med = lambda v: float(np.median(v))
    for cfg in args.configs.split(","):
        base = S.bunny_scene(n=CONFIGS[cfg], bvh="gpu", device=args.device)
        moves = {"rotate2": lambda: rotate(base.tri, base.norm, 2.0), "sine1": lambda: (sine(base.tri, 0.01), None),
                 "sine10": lambda: (sine(base.tri, 0.1), None)}
        for name, mk in moves.items():
            tri, norm = mk()
            sc = Scene(base, args.device)
            pt = PathTracer(sc, W, H, device=args.device, num_bounces=8)
            pt.prepare()
            sah0 = sc.sah_cost()
            d_tri = torch.from_numpy(tri).to(f"cuda:{args.device}")
            d_norm = None if norm is None else torch.from_numpy(norm).to(f"cuda:{args.device}")
            sc.update_geometry(base.tri, base.norm)  # the first update makes the device copies: not timed
            sc2 = Scene(base, args.device)  # the scene that is rebuilt in place, with a target that lives through it
            pt2 = PathTracer(sc2, W, H, device=args.device, num_bounces=8)
            pt2.prepare()
            leaf = np.arange(base.n_tris, dtype=np.int64)  # sc2's leaf order in terms of the base's
            in_order = lambda a, k: None if a is None else np.ascontiguousarray(a.reshape(-1, k)[leaf]).reshape(-1)
            ih, idv, split = [], [], {}
            th, td, km, rb, parts, launches = [], [], [], [], [], 0
            fresh, text = None, obj_of(tri).encode()
            for _ in range(args.reps):
                t0 = time.perf_counter(); sc.update_geometry(tri, norm); th.append(time.perf_counter() - t0)
                t0 = time.perf_counter(); sc.update_geometry(d_tri, d_norm); td.append(time.perf_counter() - t0)
                ms, launches = sc.last_update_ms()
                km.append(ms)
                t2h, n2h = in_order(tri, 9), in_order(norm, 27)
                t0 = time.perf_counter(); o = sc2.rebuild_geometry(t2h, n2h); ih.append(time.perf_counter() - t0)
                leaf = leaf[o.astype(np.int64)]
                t2d = torch.from_numpy(in_order(tri, 9)).to(f"cuda:{args.device}")
                n2d = None if norm is None else torch.from_numpy(in_order(norm, 27)).to(f"cuda:{args.device}")
                torch.cuda.synchronize(args.device)
                t0 = time.perf_counter(); o = sc2.rebuild_geometry(t2d, n2d); idv.append(time.perf_counter() - t0)
                leaf = leaf[o.cpu().numpy()]
                split = sc2.last_rebuild_ms()
                if fresh:
                    fresh[2].close(); fresh[1].close()
                fresh = rebuild(base, text, args.device, W, H)
                rb.append(fresh[0]); parts.append(fresh[3])
            nbytes = moved_bytes(base, norm is not None, sc.two_level_nodes()[0])
            out = {"config": cfg, "move": name, "triangles": base.n_tris, "depth": base.depth,
                   "update_host_s": med(th), "update_device_s": med(td), "update_kernel_ms": med(km), "launches": launches,
                   "bytes": nbytes, "gb_s": nbytes / (med(km) * 1e-3) / 1e9, "hbm_frac": nbytes / (med(km) * 1e-3) / 1e9 / HBM_PEAK_GBS,
                   "rebuild_s": med(rb), "rebuild_parts_s": [round(float(x), 4) for x in np.median(np.array(parts), axis=0)], "rebuild_over_update_device": med(rb) / med(td),
                   "inplace_host_s": med(ih), "inplace_device_s": med(idv), "inplace_split": split,
                   "inplace_device_range_s": [min(idv), max(idv)], "rebuild_range_s": [min(rb), max(rb)],
                   "rebuild_over_inplace_device": med(rb) / med(idv),
                   "sah_before": sah0, "sah_refit": sc.sah_cost(), "sah_inplace": sc2.sah_cost(), "sah_fresh": fresh[1].sah_cost()}
            if not args.no_rate:
                out["msamples_refit"] = rate(pt)
                out["msamples_inplace"] = rate(pt2)
                out["msamples_fresh"] = rate(fresh[2])
            fresh[2].close(); fresh[1].close(); pt.close(); sc.close(); pt2.close(); sc2.close()
            print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
