#!/usr/bin/env python3
"""Bloom: what the pyramid costs and what it does to the picture.

  --timing   at 1920 x 1080, HIP events, best of 5 after a warm-up, one process: the down chain, the tail and the up chain in the
             per-level form (0) and in the fused-tail form (1) at both tail thresholds (2048: 60 x 34 and below in k_bloom_tail;
             8192: 120 x 68 too), k_draw_bloom, and k_draw measured in the same run with the mode off (events around fspt_draw's
             launch are not exported, so k_draw is timed as the k_draw_auto behind a metering: the same body)
  (default)  informational: an off / on pair of PNGs of lights_ref.scene_e3 and the mean drawn luma (0..255) of each

usage: python tools/bloom_quality.py [--timing] [--out PREFIX]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def set_cam(pt, cam):
    pt.set_camera(**{k: cam[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")})


def drawn_luma(rgba8):
    return float((rgba8[..., :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])).mean())


def timing(arrays, camera, w=1920, h=1080):
    """[(label, down ms, tail ms, up ms, k_draw_bloom ms)], k_draw ms"""
    from fspt_amd import PathTracer, bloom_set_form, bloom_set_tail_texels
    pt = PathTracer(arrays, w, h, num_bounces=4)
    set_cam(pt, camera)
    pt.render(8)
    pt.set_auto_exposure(True)  # mode off: the draw behind a metering is k_draw's body, and its events are exported
    k_draw = 1e9
    for k in range(6):
        pt.draw()
        if k:
            k_draw = min(k_draw, pt.exposure_last_ms()[2])
    pt.set_auto_exposure(False)
    pt.set_bloom(True)
    rows = []
    try:
        for label, form, texels in (("per level", 0, 0), ("tail from 60 x 34", 1, 2048), ("tail from 120 x 68", 1, 8192)):
            bloom_set_form(form); bloom_set_tail_texels(texels)
            best = [1e9] * 4
            for k in range(6):
                pt.draw()
                if k:
                    best = [min(b, m) for b, m in zip(best, pt.bloom_last_ms())]
            rows.append((label, *best))
    finally:
        bloom_set_form(0); bloom_set_tail_texels(0)
    pt.close(); pt.scene.close()
    return rows, k_draw


def pictures(prefix, w=480, h=270):
    import lights_ref as LR
    from PIL import Image
    from fspt_amd import PathTracer, scene as S
    pt = PathTracer(LR.scene_e3(), w, h, num_bounces=4)
    set_cam(pt, dict(S.BUNNY_CAMERA))
    pt.render(32)
    pt.set_auto_exposure(True)
    out = []
    for name, on in (("off", False), ("on", True)):
        pt.set_bloom(on)
        img = pt.draw()
        Image.fromarray(img[::-1, :, :3].copy()).save(f"{prefix}_{name}.png")
        out.append((name, drawn_luma(img)))
    pt.close(); pt.scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--out", default="bloom")
    args = ap.parse_args()
    from fspt_amd import scene as S
    if args.timing:
        rows, k_draw = timing(S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0), dict(S.BUNNY_CAMERA))
        print("| form, 1920 x 1080 | down chain ms | tail ms | up chain ms | chain ms | k_draw_bloom ms | k_draw ms | chain / k_draw |")
        print("|---|---|---|---|---|---|---|---|")
        for label, d, t, u, b in rows:
            print("| %s | %.4f | %.4f | %.4f | %.4f | %.4f | %.4f | %.2f |" % (label, d, t, u, d + t + u, b, k_draw, (d + t + u) / k_draw))
        return
    for name, luma in pictures(args.out):
        print("bloom %s: mean drawn luma %.1f (%s_%s.png)" % (name, luma, args.out, name))


if __name__ == "__main__":
    main()
