#!/usr/bin/env python3
"""tools/cloth_demo.py - a flag waves over a floor; a few torch operations compute its vertex positions on the device every
frame and every frame is one Scene.update_vertices: no vertex crosses the bus, and no normal is computed by
the host after the first frame.

    python tools/cloth_demo.py --frames 12 --out 'cloth_{frame}.png' [--grid 48] [--samples 32] [--size 320x240] [--flat] [--temporal]

The flag is a grid of --grid x --grid vertices held along its left edge; a vertex is displaced along z by a travelling wave
whose amplitude grows with its distance from the pole.  The floor has no vt and is therefore static.  --temporal blends
every frame with the reprojected frames before it (motion_begin, update_vertices, temporal_accumulate: the motion vectors
come from the derived triangles)."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLOOR_OBJ = "v 0.5 0.0 0.5\nv 0.5 0.0 -0.5\nv -0.5 0.0 -0.5\nv -0.5 0.0 0.5\nf 1 3 2\nf 3 1 4\n"  # no vt: static


def flag_obj(n):
    v, vt, f = [], [], []
    for y in range(n):
        for x in range(n):
            v.append("v %r %r 0.0" % (float(np.float32(-0.8 + 1.6 * x / (n - 1))), float(np.float32(-0.1 + 0.9 * y / (n - 1)))))
            vt.append("vt %r %r" % (x / (n - 1), y / (n - 1)))
    for y in range(n - 1):
        for x in range(n - 1):
            a = y * n + x + 1
            b, c, d = a + 1, a + n, a + n + 1
            f += ["f %d/%d %d/%d %d/%d" % (a, a, b, b, d, d), "f %d/%d %d/%d %d/%d" % (a, a, d, d, c, c)]
    return "\n".join(v + vt + f) + "\n"


def build(n, flat):
    from fspt_amd import scene as S
    env, w, h = S.synthetic_env(256, 128)
    props = [{"path": "flag.obj", "diffuse": [0.8, 0.3, 0.25], "emittance": [0, 0, 0], "normals": "flat" if flat else "smooth"},
             {"path": "floor.obj", "scale": 4.0, "translate": [0, -0.5, 0], "diffuse": [0.7, 0.7, 0.65], "emittance": [0, 0, 0]}]
    return S.build_scene(props, {"flag.obj": flag_obj(n), "floor.obj": FLOOR_OBJ}, env=env, env_w=w, env_h=h, bvh="gpu", keep_order=True, keep_mesh=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default="cloth_{frame}.png")
    ap.add_argument("--grid", type=int, default=48)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--size", default="320x240")
    ap.add_argument("--flat", action="store_true")
    ap.add_argument("--temporal", action="store_true")
    args = ap.parse_args()
    import torch
    from PIL import Image
    from fspt_amd import PathTracer
    w, h = (int(x) for x in args.size.split("x"))
    arrays = build(args.grid, args.flat)
    pt = PathTracer(arrays, w, h, num_bounces=4)
    pt.set_camera(P=[0.0, 0.35, 2.2], I=[0.0, -0.1, -1.0], fov_scale=1.0, focal_depth=2.2, aperture=0.0, env_theta=0.0)
    pt.set_mesh()
    rest = torch.from_numpy(arrays.meta["vertices"]).to(f"cuda:{pt.scene.device}")  # the only upload
    reach = (rest[:, 0] + 0.8) / 1.6  # 0 at the pole
    flag = torch.arange(rest.shape[0], device=rest.device) < args.grid * args.grid  # (the floor's vertices follow; they are static)
    print(f"{arrays.n_tris} triangles, {arrays.meta['n_vertices']} vertices, {pt.last_mesh['bytes']} bytes of mesh")
    for f in range(args.frames):
        phase = 2 * math.pi * f / max(args.frames, 1)
        pos = rest.clone()
        wave = torch.sin(7.0 * rest[:, 0] - phase) * 0.12 + torch.sin(4.0 * rest[:, 1] + 2.0 * phase) * 0.04
        pos[:, 2] = torch.where(flag, wave * reach, rest[:, 2])
        if args.temporal:
            pt.scene.motion_begin()
        pt.update_vertices(pos.contiguous())
        pt.clear(); pt.seed(1 + f); pt.render(args.samples)
        if args.temporal:
            pt.temporal_accumulate(read=False)
            rgba = pt.temporal_draw(1.0, 1.0)
        else:
            rgba = pt.draw(1.0)
        path = args.out.format(frame=f)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        Image.fromarray(rgba[::-1, :, :3].copy()).save(path)
        ms = pt.last_mesh
        print(f"frame {f}: {path}  (derive {ms['derive_ms']:.3f} ms + refit {ms['refit_ms']:.3f} ms, {ms['launches']} launches)")
    if args.temporal:
        pt.scene.motion_end()
    pt.close(); pt.scene.close()


if __name__ == "__main__":
    main()
