#!/usr/bin/env python3
"""tools/skin_bench.py - Scene.update_skin in both joint-table forms against the two ways to deform the same mesh without it
(DESIGN 8.16).

    python tools/skin_bench.py --reps 3 [--configs c2,c3] [--joints 16,64,256,1024] [--ids coherent,hashed]

Per config (c2: 69 316 triangles, c3: 1 002 256; the tree built on the GPU), joint count and id layout one JSON line.  The
skin has rest normals and no morph targets: k_skin_transform then moves 360 bytes per triangle (24 ids + 48 weights + 144
rest read, 144 written).  Id layouts: "coherent" - a corner's four joints are the four neighbours of (leaf position x
n_joints / T), what a skinned character looks like after a spatial sort; "hashed" - four joints from a hash of the corner,
the worst case for the gather.  The frame turns joint k by (2 + k % 5) degrees per rep about y and shifts it.
Timed in one process, interleaved rep by rep, the first call of every path not timed; per column the median and the values:
  skin_s[form]       Scene.update_skin: 48 bytes per joint up, k_skin_transform, the refit (form 0: the joint table read from
                     global memory, form 1: staged per block in LDS - fspt_skin_set_form)
  skin_ms[form], refit_ms, launches     its parts on the GPU (Scene.last_skin)
  skin_gb_s[form], hbm_frac[form]       360 bytes per triangle over skin_ms; against bench.py's 8 TB/s
  numpy_host_s (numpy_s + host_update_s) the same blend and transform in numpy (float32 einsum over all corners) + the host
                     form of Scene.update_geometry (144 bytes per triangle up, the refit)      ("coherent" lines only)
  torch_device_s     the same as torch einsums on the device + the device form of update_geometry   ("coherent" lines only)"""
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
BYTES_PER_TRI = 24 + 48 + 144 + 144


def skin_ids(T, n_joints, layout):
    """joints [T, 3, 4] uint16, weights [T, 3, 4] float32 (each corner's sum to 1)"""
    c = np.arange(T * 3, dtype=np.uint64)
    if layout == "coherent":
        base = (c // np.uint64(3)) * np.uint64(n_joints) // np.uint64(T)
        ids = (base[:, None] + np.arange(4, dtype=np.uint64)[None, :]) % np.uint64(n_joints)
    else:
        k = c[:, None] * np.uint64(4) + np.arange(4, dtype=np.uint64)[None, :]
        ids = (((k * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(0xFFFFFFFF)) % np.uint64(n_joints)
    raw = ((c[:, None] * np.uint64(40503) + np.arange(4, dtype=np.uint64)[None, :] * np.uint64(977)) % np.uint64(1000)).astype(np.float64) + 1.0
    w = (raw / raw.sum(1, keepdims=True)).astype(np.float32)
    return ids.astype(np.uint16).reshape(T, 3, 4), w.reshape(T, 3, 4)


def frame(n_joints, k):
    from fspt_amd import scene as S
    xf = np.tile(np.eye(3, 4), (n_joints, 1, 1))
    for j in range(n_joints):
        xf[j, :, :3] = S._rotation_matrix([0.0, 1.0, 0.0], np.radians((2.0 + j % 5) * k))
        xf[j, :, 3] = [0.001 * k * (j % 7), 0.0, -0.0005 * k]
    return xf.reshape(n_joints, 12).astype(np.float32)


def numpy_lbs(j, w, tri, norm, xf):
    J = xf.reshape(-1, 3, 4)
    B = np.einsum("ck,ckij->cij", w, J[j])
    v = np.einsum("cij,cj->ci", B[:, :, :3], tri.reshape(-1, 3)) + B[:, :, 3]
    f = np.einsum("cij,cvj->cvi", B[:, :, :3], norm.reshape(-1, 3, 3))  # (rotations: D = N = B's 3 x 3 up to the weights)
    return v.astype(np.float32).reshape(-1), f.astype(np.float32).reshape(-1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--configs", default="c2,c3")
    ap.add_argument("--joints", default="16,64,256,1024")
    ap.add_argument("--ids", default="coherent,hashed")
    args = ap.parse_args()
    import torch
    from fspt_amd import Scene, skin_set_form
    from fspt_amd import scene as S
    med = lambda x: float(np.median(x))
    for cfg in args.configs.split(","):
        arrays = S.bunny_scene(n=CONFIGS[cfg], env_size=(64, 32), bvh="gpu")
        T = arrays.n_tris
        K, Hs, D = Scene(arrays), Scene(arrays), Scene(arrays)
        d_tri = torch.from_numpy(arrays.tri).to("cuda:0").reshape(-1, 3)
        d_norm = torch.from_numpy(arrays.norm).to("cuda:0").reshape(-1, 3, 3)
        for layout in args.ids.split(","):
            for nj in (int(x) for x in args.joints.split(",")):
                joints, weights = skin_ids(T, nj, layout)
                K.set_skin(joints, weights, arrays.tri, arrays.norm, n_joints=nj)
                others = layout == "coherent"
                jc, wc = joints.reshape(-1, 4).astype(np.int64), weights.reshape(-1, 4)
                d_j, d_w = torch.from_numpy(jc).to("cuda:0"), torch.from_numpy(wc).to("cuda:0")

                def torch_lbs(xf):
                    J = torch.from_numpy(xf).to("cuda:0").reshape(-1, 3, 4)
                    B = torch.einsum("ck,ckij->cij", d_w, J[d_j])
                    v = torch.einsum("cij,cj->ci", B[:, :, :3], d_tri) + B[:, :, 3]
                    f = torch.einsum("cij,cvj->cvi", B[:, :, :3], d_norm)
                    return v.reshape(-1).contiguous(), f.reshape(-1).contiguous()

                ts, tk, tr, nl = ([], []), ([], []), [], 0
                tn, th, td = [], [], []
                for k in range(args.reps + 1):
                    xf = frame(nj, k + 1)
                    for form in (0, 1):
                        skin_set_form(form)
                        t0 = time.perf_counter(); K.update_skin(xf); a = time.perf_counter() - t0
                        ms = K.last_skin
                        if k:
                            ts[form].append(a); tk[form].append(ms["skin_ms"]); tr.append(ms["refit_ms"]); nl = ms["launches"]
                    skin_set_form(0)
                    if not others:
                        continue
                    t0 = time.perf_counter(); tri, norm = numpy_lbs(jc, wc, arrays.tri, arrays.norm, xf); b = time.perf_counter() - t0
                    t0 = time.perf_counter(); Hs.update_geometry(tri, norm); c = time.perf_counter() - t0
                    torch.cuda.synchronize()
                    t0 = time.perf_counter(); D.update_geometry(*torch_lbs(xf)); d = time.perf_counter() - t0
                    if k:
                        tn.append(b); th.append(c); td.append(d)
                gbs = [T * BYTES_PER_TRI / (med(tk[f]) * 1e-3) / 1e9 for f in (0, 1)]
                line = dict(config=cfg, triangles=T, joints=nj, ids=layout, reps=args.reps,
                            skin_s=[med(ts[0]), med(ts[1])], skin_s_all=[ts[0], ts[1]],
                            skin_ms=[med(tk[0]), med(tk[1])], skin_ms_all=[tk[0], tk[1]], refit_ms=med(tr), launches=nl,
                            skin_gb_s=gbs, hbm_frac=[g / HBM_PEAK_GBS for g in gbs], skin_bytes=K.last_skin["bytes"])
                if others:
                    line.update(numpy_s=med(tn), host_update_s=med(th), numpy_host_s=med(np.add(tn, th)), numpy_host_s_all=list(np.add(tn, th)),
                                torch_device_s=med(td), torch_device_s_all=td, skin_over_host=med(np.add(tn, th)) / med(ts[0]))
                print(json.dumps(line), flush=True)
        K.close(); Hs.close(); D.close()


if __name__ == "__main__":
    main()
