#!/usr/bin/env python3
"""Auto-exposure: what the metering costs and what it does to the picture.

  --timing   k_exposure_histogram in both forms (0 = one LDS atomic per pixel, 1 = the first active lane's bin counted by a
             ballot), k_exposure_resolve and the k_draw_auto behind them at 1920 x 1080, HIP events, best of 5 after a warm-up,
             on a constant image (every lane in one bin) and on a rendered frame of the bunny scene; the metering / k_draw ratio
  (default)  informational: mean drawn luma (0..255, Rec.709 of the RGBA8 frame) of the project's test scenes at exposure 1 and
             under auto-exposure, and over DESIGN 8.10's light sequence (lights_ref.scene_e3, env_theta turned a quarter after 16
             frames) at exposure 1, with instant adaptation and with render_sequence's SEQUENCE_ADAPT

usage: python tools/exposure_quality.py [--timing]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LIGHT_BEFORE, LIGHT_AFTER, TICKS = 16, 8, 4


def set_cam(pt, cam):
    pt.set_camera(**{k: cam[k] for k in ("P", "I", "fov_scale", "env_theta", "focal_depth", "aperture")})


def drawn_luma(rgba8):
    return float((rgba8[..., :3].astype(np.float64) @ np.array([0.2126, 0.7152, 0.0722])).mean())


def timing(arrays, camera, w=1920, h=1080):
    """input -> form -> (histogram ms, resolve ms, k_draw_auto ms), each the best of 5 after a warm-up, in one process"""
    import torch
    from fspt_amd import PathTracer, exposure_set_form
    pt = PathTracer(arrays, w, h, num_bounces=4)
    set_cam(pt, camera)
    pt.set_auto_exposure(True)
    flat = torch.empty((h, w, 4), dtype=torch.float32, device="cuda:0")
    flat[..., 0], flat[..., 1], flat[..., 2], flat[..., 3] = 0.5, 0.25, 0.75, 1.0
    torch.cuda.synchronize()
    out = {}
    try:
        for name in ("rendered", "constant"):
            if name == "rendered":
                pt.render(8)
            else:
                pt.bind_accumulator(flat.data_ptr(), keep=flat)
            out[name] = {}
            for form in (0, 1):
                exposure_set_form(form)
                best = [1e9, 1e9, 1e9]
                for k in range(6):
                    pt.draw()
                    if k:
                        best = [min(b, m) for b, m in zip(best, pt.exposure_last_ms())]
                out[name][form] = tuple(best)
    finally:
        exposure_set_form(0)
    pt.close(); pt.scene.close()
    return out


def scenes_table(w=480, h=270):
    import lights_ref as LR
    from fspt_amd import PathTracer, scene as S
    rows = []
    cam = dict(S.BUNNY_CAMERA)
    for name, arrays in (("bunny n=8", S.bunny_scene(n=8, env_size=(64, 32))), ("bunny n=24, sun", S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0)),
                         ("lights E3", LR.scene_e3())):
        pt = PathTracer(arrays, w, h, num_bounces=4)
        set_cam(pt, cam)
        pt.render(16)
        fixed = drawn_luma(pt.draw())
        pt.set_auto_exposure(True)
        auto = drawn_luma(pt.draw())
        rows.append((name, fixed, auto, float(pt.exposure()[0])))
        pt.close(); pt.scene.close()
    return rows


def light_sequence(w=480, h=270):
    """mean drawn luma per frame over the change of light: fixed exposure 1, auto with instant adaptation, auto with SEQUENCE_ADAPT"""
    import lights_ref as LR
    from fspt_amd import PathTracer, scene as S
    from fspt_amd.scene_file import SEQUENCE_ADAPT
    cam = dict(S.BUNNY_CAMERA)
    pt = {k: PathTracer(LR.scene_e3(), w, h, num_bounces=4) for k in ("fixed", "instant", "slow")}
    pt["instant"].set_auto_exposure(True)
    pt["slow"].set_auto_exposure(True, adapt_up=SEQUENCE_ADAPT, adapt_down=SEQUENCE_ADAPT)
    rows = []
    for f in range(LIGHT_BEFORE + LIGHT_AFTER):
        c = dict(cam, env_theta=cam["env_theta"] + (np.pi / 2 if f >= LIGHT_BEFORE else 0.0))
        row = [f]
        for k, p in pt.items():
            set_cam(p, c)
            p.clear(); p.seed(1 + f); p.render(TICKS)
            row.append(drawn_luma(p.draw()))
        row.append(float(pt["slow"].exposure()[0]))
        rows.append(row)
    for p in pt.values():
        p.close(); p.scene.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    args = ap.parse_args()
    from fspt_amd import scene as S
    if args.timing:
        r = timing(S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0), dict(S.BUNNY_CAMERA))
        print("| input, 1920 x 1080 | form | k_exposure_histogram ms | k_exposure_resolve ms | k_draw_auto ms | metering / k_draw |")
        print("|---|---|---|---|---|---|")
        for name, v in r.items():
            for form, (hm, rm, dm) in v.items():
                print("| %s | %d | %.4f | %.4f | %.4f | %.3f |" % (name, form, hm, rm, dm, (hm + rm) / dm))
        return
    print("| scene | mean drawn luma, exposure 1 | auto | metered exposure |")
    print("|---|---|---|---|")
    for row in scenes_table():
        print("| %s | %.1f | %.1f | %.4f |" % row)
    print("| frame | exposure 1 | auto, instant | auto, SEQUENCE_ADAPT | its exposure |")
    print("|---|---|---|---|---|")
    for row in light_sequence():
        print("| %d | %.1f | %.1f | %.1f | %.4f |" % tuple(row))


if __name__ == "__main__":
    main()
