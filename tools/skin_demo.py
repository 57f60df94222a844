#!/usr/bin/env python3
"""tools/skin_demo.py - a procedurally skinned tube bends and bulges over a floor, every frame one Scene.update_skin
(DESIGN 8.16): no triangle is computed or uploaded by the host after the first frame.

    python tools/skin_demo.py --frames 12 --out 'skin_{frame}.png' [--joints 5] [--samples 32] [--size 320x240] [--temporal]

The tube stands on the floor along y; joint 0 holds the floor (identity), joints 1 .. J sit at equal heights and form a chain,
each turning about z around its own height relative to its parent.  A corner is weighted between the two joints next to its
height; one morph target swells the tube around its middle.  --temporal blends every frame with the reprojected frames before
it (motion_begin, update_skin, temporal_accumulate: the motion vectors come from the skinned triangles)."""
import argparse
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

Y0, Y1, RADIUS = -0.5, 0.7, 0.12


def tube_obj(rings=24, sides=16):
    v, f = [], []
    for r in range(rings + 1):
        y = Y0 + (Y1 - Y0) * r / rings
        for s in range(sides):
            a = 2 * math.pi * s / sides
            v.append("v %.6f %.6f %.6f" % (RADIUS * math.cos(a), y, RADIUS * math.sin(a)))
    for r in range(rings):
        for s in range(sides):
            a, b = r * sides + s + 1, r * sides + (s + 1) % sides + 1
            c, d = a + sides, b + sides
            f += ["f %d %d %d" % (a, c, b), "f %d %d %d" % (b, c, d)]
    return "\n".join(v + f) + "\n"


def build(n_joints):
    """(arrays, joints [T, 3, 4], weights [T, 3, 4], morph [1, T, 9], joint heights)"""
    from fspt_amd import scene as S
    env, w, h = S.synthetic_env(256, 128)
    props = [{"path": "tube.obj", "scale": 1.0, "translate": [0, 0, 0], "diffuse": [0.8, 0.35, 0.25], "emittance": [0, 0, 0], "normals": "smooth"},
             {"path": "quad.obj", "scale": 3.0, "translate": [0, Y0, 0], "diffuse": [0.7, 0.7, 0.65], "emittance": [0, 0, 0]}]
    arrays = S.build_scene(props, {"tube.obj": tube_obj(), "quad.obj": S.QUAD_OBJ}, env=env, env_w=w, env_h=h, bvh="gpu", keep_order=True)
    T = arrays.n_tris
    pos = arrays.tri.reshape(T * 3, 3).astype(np.float64)
    tube = np.repeat(arrays.meta["tri_part"] == 0, 3)
    heights = Y0 + (Y1 - Y0) * np.arange(n_joints) / n_joints  # joint k + 1 pivots at heights[k]
    u = np.clip((pos[:, 1] - Y0) / (Y1 - Y0), 0.0, 1.0) * n_joints - 0.5  # where between the joints a corner sits
    lo = np.clip(np.floor(u), 0, n_joints - 1).astype(np.int64)
    hi = np.clip(lo + 1, 0, n_joints - 1)
    frac = np.clip(u - lo, 0.0, 1.0)
    joints = np.zeros((T * 3, 4), np.uint16)
    weights = np.zeros((T * 3, 4), np.float32)
    joints[tube, 0], joints[tube, 1] = lo[tube] + 1, hi[tube] + 1
    weights[tube, 0], weights[tube, 1] = 1.0 - frac[tube], frac[tube]
    weights[~tube, 0] = 1.0  # the floor: joint 0
    radial = pos * [1.0, 0.0, 1.0] / RADIUS
    bump = np.exp(-((pos[:, 1] - 0.5 * (Y0 + Y1)) / 0.18) ** 2)
    morph = np.where(tube[:, None], radial * bump[:, None] * 0.12, 0.0).astype(np.float32)
    return arrays, joints.reshape(T, 3, 4), weights.reshape(T, 3, 4), morph.reshape(1, T, 9), heights


def skeleton(heights, bend):
    """[1 + J, 12] float32: joint 0 the identity, joint k + 1 = its parent's matrix x a turn by `bend` about z around heights[k]"""
    out = [np.eye(4)]
    m = np.eye(4)
    c, s = math.cos(bend), math.sin(bend)
    for y in heights:
        local = np.array([[c, -s, 0, s * y], [s, c, 0, y - c * y], [0, 0, 1, 0], [0, 0, 0, 1]], np.float64)
        m = m @ local
        out.append(m.copy())
    return np.stack(out)[:, :3, :].reshape(-1, 12).astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=12)
    ap.add_argument("--out", default="skin_{frame}.png")
    ap.add_argument("--joints", type=int, default=5)
    ap.add_argument("--samples", type=int, default=32)
    ap.add_argument("--size", default="320x240")
    ap.add_argument("--temporal", action="store_true")
    args = ap.parse_args()
    from PIL import Image
    from fspt_amd import PathTracer
    w, h = (int(x) for x in args.size.split("x"))
    arrays, joints, weights, morph, heights = build(args.joints)
    pt = PathTracer(arrays, w, h, num_bounces=4)
    pt.set_camera(P=[0.0, 0.35, 2.2], I=[0.0, -0.1, -1.0], fov_scale=1.0, focal_depth=2.2, aperture=0.0, env_theta=0.0)
    pt.set_skin(joints, weights, morph=morph)
    print(f"{arrays.n_tris} triangles, {args.joints + 1} joints, 1 morph target, {pt.last_skin['bytes']} bytes of skin")
    for f in range(args.frames):
        phase = 2 * math.pi * f / max(args.frames, 1)
        xf = skeleton(heights, 0.25 * math.sin(phase))
        if args.temporal:
            pt.scene.motion_begin()
        pt.update_skin(xf, np.float32([0.5 - 0.5 * math.cos(phase)]))
        pt.clear(); pt.seed(1 + f); pt.render(args.samples)
        if args.temporal:
            pt.temporal_accumulate(read=False)
            rgba = pt.temporal_draw(1.0, 1.0)
        else:
            rgba = pt.draw(1.0)
        path = args.out.format(frame=f)
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        Image.fromarray(rgba[::-1, :, :3].copy()).save(path)
        ms = pt.last_skin
        print(f"frame {f}: {path}  (skin {ms['skin_ms']:.3f} ms + refit {ms['refit_ms']:.3f} ms, {ms['launches']} launches)")
    if args.temporal:
        pt.scene.motion_end()
    pt.close(); pt.scene.close()


if __name__ == "__main__":
    main()
