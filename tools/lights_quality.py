"""Quality and cost of next-event estimation of emissive triangles (fspt_target_set_lights) on scene E1 of
tests/lights_ref.py (a small flat-colour emitter, no environment map), 4 bounces.

    python tools/lights_quality.py [--reps 3] [--width 1920 --height 1080] [--out lights_quality.json]

Quality: relative MSE (err^2 / (ref^2 + 0.01)) at 16 spp with the mode on and off, against a 4096-spp
frame with it off, averaged over 4 seeds; and at EQUAL TIME: the mode-on error scaled by its time per sample over the
mode-off one (relative MSE falls as 1 / spp).  Cost: Gsamples/s of render(128) on and off, interleaved over --reps, timed
as tools/present_bench.py times (sync before and after, perf_counter).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fspt_amd import PathTracer, scene as S  # noqa: E402
import lights_ref as R  # noqa: E402

SEEDS = 4


def rel_mse(img, ref):
    e = img[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.mean(e * e / (ref[..., :3].astype(np.float64) ** 2 + 0.01)))


def make(arrays, W, H, on, seed):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.seed(seed + 1)
    if on:
        pt.set_lights("emitters")
    return pt


def render(arrays, W, H, on, seed, spp):
    pt = make(arrays, W, H, on, seed)
    pt.render(spp)
    img = pt.readRadiance()
    pt.close()
    return img


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--spp", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arrays = R.scene_e1()
    W, H = a.width, a.height
    ref = render(arrays, W, H, False, 1000, 4096)
    err = {m: float(np.mean([rel_mse(render(arrays, W, H, m == "on", s, a.spp), ref) for s in range(SEEDS)])) for m in ("off", "on")}
    rate = {"off": [], "on": []}
    pts = {m: make(arrays, W, H, m == "on", 7) for m in ("off", "on")}
    for m in ("off", "on"):
        pts[m].render(8)  # warm-up (table built, kernels loaded)
        pts[m].sync()
    for _ in range(a.reps):
        for m in ("off", "on"):
            pts[m].sync()
            t0 = time.perf_counter()
            pts[m].render(128)
            pts[m].sync()
            rate[m].append(W * H * 128 / (time.perf_counter() - t0) / 1e9)
    for p in pts.values():
        p.close()
    g = {m: float(np.median(v)) for m, v in rate.items()}
    res = {"scene": "E1", "width": W, "height": H, "spp": a.spp, "relmse_off": err["off"], "relmse_on": err["on"],
           "ratio_equal_spp": err["on"] / err["off"], "ratio_equal_time": err["on"] / err["off"] * g["off"] / g["on"],
           "gsamples_off": g["off"], "gsamples_on": g["on"], "cost": g["off"] / g["on"] - 1.0, "rates": rate}
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
