"""Quality and cost of the Owen-scrambled Sobol sampler against the reference sampler (fspt_target_set_sampler).

    python tools/sampler_quality.py [--reps 3] [--out sampler_quality.json]

Quality: relative MSE (err^2 / (ref^2 + 0.01)) at 4, 16 and 64 spp for both samplers, against a 4096-spp
reference-sampler frame, averaged over 4 seeds, raw and after denoise() with its defaults - the medium test scene at
320x240 and bench C2 at 480x270.  Cost: Gsamples/s of render(128) on C2 at 1920x1080 for both samplers, interleaved over
--reps, timed as tools/present_bench.py times (sync before and after, perf_counter).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fspt_amd import PathTracer, scene as S  # noqa: E402

SEEDS = 4


def rel_mse(img, ref):
    e = img[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.mean(e * e / (ref[..., :3].astype(np.float64) ** 2 + 0.01)))


def make(arrays, W, H, cam, sampler, seed, nb):
    pt = PathTracer(arrays, W, H, num_bounces=nb)
    pt.set_camera(**cam)
    pt.seed(seed + 1)
    if sampler == "sobol":
        pt.set_sampler("sobol", seed)
    return pt


def quality(arrays, W, H, cam, nb):
    pt = make(arrays, W, H, cam, "reference", 1000, nb)
    pt.render(4096)
    ref = pt.readRadiance()
    pt.features(8, 1)
    pt.close()
    out = {}
    for spp in (4, 16, 64):
        for smp in ("reference", "sobol"):
            raw, den = [], []
            for seed in range(SEEDS):
                pt = make(arrays, W, H, cam, smp, seed, nb)
                pt.render(spp)
                raw.append(rel_mse(pt.readRadiance(), ref))
                pt.features(8, 1)
                den.append(rel_mse(pt.denoise(), ref))
                pt.close()
            out["%s_%d" % (smp, spp)] = {"raw": float(np.mean(raw)), "denoised": float(np.mean(den))}
        for k in ("raw", "denoised"):
            out["ratio_%d_%s" % (spp, k)] = out["sobol_%d" % spp][k] / out["reference_%d" % spp][k]
    return out


def throughput(arrays, cam, nb, reps):
    W, H, n = 1920, 1080, 128
    pts = {smp: make(arrays, W, H, cam, smp, 0, nb) for smp in ("reference", "sobol")}
    gs = {smp: [] for smp in pts}
    for pt in pts.values():
        pt.render(8)  # warm-up: allocation, tuners
        pt.sync()
    for _ in range(reps):
        for smp, pt in pts.items():
            pt.clear(); pt.sync()
            t0 = time.perf_counter()
            pt.render(n)
            pt.sync()
            gs[smp].append(W * H * n / (time.perf_counter() - t0) / 1e9)
    for pt in pts.values():
        pt.close()
    best = {smp: max(v) for smp, v in gs.items()}
    return {"gsamples_per_s": gs, "best": best, "cost": 1.0 - best["sobol"] / best["reference"]}


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    medium = S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0)
    cam = dict(S.BUNNY_CAMERA)
    c2 = S.bunny_scene(n=76)  # bench.py C2: 70 k triangles
    res = {"medium_320x240": quality(medium, 320, 240, cam, 8), "c2_480x270": quality(c2, 480, 270, cam, 8),
           "c2_1080p": throughput(c2, cam, 8, a.reps)}
    print(json.dumps(res, indent=1))
    if a.out:
        json.dump(res, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
