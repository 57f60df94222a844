#!/usr/bin/env python3
"""tools/pose_bench.py - Scene.update_transforms against the two ways to make the same move without it.

    python tools/pose_bench.py --reps 3 [--configs c2,c3]

Per config (c2: 69 316 triangles, c3: 1 002 256; the tree built on the GPU, one part per prop) the move is one rigid matrix
per prop - the ball turns by 2 degrees per rep and shifts, the quads stay.  One JSON line with, medians of --reps, timed in
one process, interleaved rep by rep (the first call of every path is a warm-up and not timed):
  transforms_s                    Scene.update_transforms: 48 bytes per prop up, k_pose_transform, the refit
  transform_ms, refit_ms, launches   its two parts on the GPU (fspt_scene_last_pose_ms)
  pose_gb_s, hbm_frac             k_pose_transform's traffic over transform_ms: per triangle 4 (part id) + 144 read + 144 written
                                  = 292 bytes; against bench.py's 8 TB/s
  numpy_host_s (numpy_s + host_update_s)   the same move in numpy (float32 matmul over all vertices and frame vectors) + the
                                  host form of Scene.update_geometry (144 bytes per triangle up, the refit)
  torch_device_s                  the same move as torch matmuls on the device + the device form of update_geometry
  transforms_over_host            numpy_host_s / transforms_s
OBJ parsing, which a host without the feature also pays per frame, is NOT counted in numpy_host_s."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = {"c2": 76, "c3": 289}
HBM_PEAK_GBS = 8000.0  # bench.py's roofline figure
BYTES_PER_TRI = 4 + 144 + 144


def matrices(k):
    """[3, 12] float32: the ball (prop 0) turned by 2 k degrees about y and shifted, the quads at rest"""
    from fspt_amd import scene as S
    xf = np.tile(np.eye(3, 4), (3, 1, 1))
    xf[0, :, :3] = S._rotation_matrix([0.0, 1.0, 0.0], np.radians(2.0 * k))
    xf[0, :, 3] = [0.01 * k, 0.0, -0.005 * k]
    return xf.reshape(3, 12).astype(np.float32)


def numpy_move(part, tri, norm, xf):
    m = xf.reshape(-1, 3, 4)
    A, t = m[:, :, :3], m[:, :, 3]
    pv, pf = np.repeat(part, 3), np.repeat(part, 9)
    v = np.einsum("nij,nj->ni", A[pv], tri.reshape(-1, 3)) + t[pv]
    f = np.einsum("nij,nj->ni", A[pf], norm.reshape(-1, 3))  # (rigid: D = N = A)
    return v.astype(np.float32).reshape(-1), f.astype(np.float32).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3")
    args = ap.parse_args()
    import torch
    from fspt_amd import Scene
    from fspt_amd import scene as S
    med = lambda x: float(np.median(x))
    for cfg in args.configs.split(","):
        arrays = S.bunny_scene(n=CONFIGS[cfg], env_size=(64, 32), bvh="gpu", keep_order=True)
        part = arrays.meta["tri_part"].astype(np.int64)
        T = arrays.n_tris
        P, Hs, D = Scene(arrays), Scene(arrays), Scene(arrays)
        P.set_pose(arrays.meta["tri_part"])
        d_tri = torch.from_numpy(arrays.tri).to("cuda:0").reshape(-1, 3)
        d_norm = torch.from_numpy(arrays.norm).to("cuda:0").reshape(-1, 3)
        d_pv = torch.from_numpy(np.repeat(part, 3)).to("cuda:0")
        d_pf = torch.from_numpy(np.repeat(part, 9)).to("cuda:0")

        def torch_move(xf):
            m = torch.from_numpy(xf).to("cuda:0").reshape(-1, 3, 4)
            A, t = m[:, :, :3], m[:, :, 3]
            v = torch.bmm(A[d_pv], d_tri.unsqueeze(-1)).squeeze(-1) + t[d_pv]
            f = torch.bmm(A[d_pf], d_norm.unsqueeze(-1)).squeeze(-1)
            return v.reshape(-1).contiguous(), f.reshape(-1).contiguous()

        tp, tk, tr, nl, tn, th, td = [], [], [], 0, [], [], []
        for k in range(args.reps + 1):
            xf = matrices(k + 1)
            t0 = time.perf_counter(); P.update_transforms(xf); a = time.perf_counter() - t0
            ms = P.last_pose_ms()
            t0 = time.perf_counter(); tri, norm = numpy_move(part, arrays.tri, arrays.norm, xf); b = time.perf_counter() - t0
            t0 = time.perf_counter(); Hs.update_geometry(tri, norm); c = time.perf_counter() - t0
            torch.cuda.synchronize()
            t0 = time.perf_counter(); D.update_geometry(*torch_move(xf)); d = time.perf_counter() - t0
            if k == 0:
                continue
            tp.append(a); tk.append(ms["transform_ms"]); tr.append(ms["refit_ms"]); nl = ms["launches"]
            tn.append(b); th.append(c); td.append(d)
        gbs = T * BYTES_PER_TRI / (med(tk) * 1e-3) / 1e9
        print(json.dumps(dict(config=cfg, triangles=T, parts=3, reps=args.reps, transforms_s=med(tp), transform_ms=med(tk), refit_ms=med(tr),
                              launches=nl, pose_gb_s=gbs, hbm_frac=gbs / HBM_PEAK_GBS, numpy_s=med(tn), host_update_s=med(th),
                              numpy_host_s=med(np.add(tn, th)), torch_device_s=med(td),
                              transforms_over_host=med(np.add(tn, th)) / med(tp))), flush=True)
        P.close(); Hs.close(); D.close()


if __name__ == "__main__":
    main()
