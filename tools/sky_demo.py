#!/usr/bin/env python3
"""A time-of-day sweep of the built-in scene under the GPU sky: one scene and one tracer, Scene.update_sky per
frame, temporal accumulation and auto-exposure across the frames - the light-side counterpart of tools/skin_demo.py.

  python tools/sky_demo.py --frames 24 --out day_{frame:03d}.png
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--out", default="sky_{frame:03d}.png")
    ap.add_argument("--width", type=int, default=640)
    ap.add_argument("--height", type=int, default=360)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--mesh-n", type=int, default=24)
    ap.add_argument("--sky-size", default="1024x512")
    ap.add_argument("--turbidity", type=float, default=2.0)
    ap.add_argument("--from-elevation", type=float, default=-6.0, help="degrees; the sun rises from here ...")
    ap.add_argument("--to-elevation", type=float, default=60.0, help="... to here, while its azimuth turns by 90 degrees")
    ap.add_argument("--no-temporal", action="store_true")
    ap.add_argument("--no-auto-exposure", action="store_true")
    args = ap.parse_args()
    import __graft_entry__ as g
    g.build()
    from PIL import Image
    from fspt_amd import PathTracer
    from fspt_amd import scene as S

    w, h = (int(v) for v in args.sky_size.lower().split("x"))
    pt = PathTracer(S.bunny_scene(n=args.mesh_n, env_size=(64, 32)), args.width, args.height, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    if not args.no_auto_exposure:
        pt.set_auto_exposure(True)
    t0 = time.perf_counter()
    light_ms = 0.0
    for f in range(args.frames):
        s = f / max(args.frames - 1, 1)
        sun = S.sun_direction(30.0 + 90.0 * s, args.from_elevation + (args.to_elevation - args.from_elevation) * s)
        pt.update_sky(sun, w, h, turbidity=args.turbidity)
        last = pt.last_sky()
        light_ms += last["sky_ms"] + last["bins_ms"] + last["tile_ms"]
        pt.clear(); pt.seed(1 + f); pt.render(args.spp)
        if args.no_temporal:
            rgba = pt.draw()
        else:
            pt.temporal_accumulate(read=False)
            rgba = pt.temporal_draw(1.0, 1.0)
        out = args.out.format(frame=f)
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        Image.fromarray(rgba[::-1, :, :3]).save(out)
    dt = time.perf_counter() - t0
    print(f"{args.frames} frames in {dt:.2f} s; the light took {light_ms / args.frames:.2f} ms of GPU time per frame ({last['n_bins']} bins at the end)")
    pt.close()


if __name__ == "__main__":
    main()
