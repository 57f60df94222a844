"""Quality and cost of adaptive sampling (fspt_render_adaptive) on c2 - the default bunny view, 1920x1080,
4 bounces.

    python tools/adaptive_quality.py [--thresholds 3e-3,1e-3,3e-4,1e-4] [--max-ticks 1024] [--out adaptive_quality.json]

For every threshold and each of 4 seeds: render_adaptive(threshold, max_ticks) and a uniform render(k) with k = the
adaptive run's samples per pixel rounded (EQUAL TOTAL SAMPLES); full-frame relative MSE (err^2 / (ref^2 + 0.01), as in
DESIGN 8.1) of both against a 4096-spp uniform frame of another seed.  EQUAL TIME: the uniform error scaled by k over
the spp the uniform rate reaches in the adaptive run's wall time (relative MSE falls as 1 / spp).  Cost: Gsamples/s of
the adaptive call (its samples / its time, rounds and read-backs included) and of render(k), medians over the seeds, timed
as tools/present_bench.py times (sync before and after, perf_counter; each tracer warmed first).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from fspt_amd import PathTracer, scene as S  # noqa: E402

SEEDS = 4


def rel_mse(img, ref):
    e = img[..., :3].astype(np.float64) - ref[..., :3]
    return float(np.mean(e * e / (ref[..., :3].astype(np.float64) ** 2 + 0.01)))


def make(arrays, W, H, seed):
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.set_camera(**S.BUNNY_CAMERA)
    pt.seed(seed + 1)
    return pt


def timed(pt, f):
    pt.sync()
    t0 = time.perf_counter()
    f()
    pt.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--thresholds", default="3e-3,1e-3,3e-4,1e-4")
    ap.add_argument("--max-ticks", type=int, default=1024)
    ap.add_argument("--min-ticks", type=int, default=64)
    ap.add_argument("--round-ticks", type=int, default=32)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    arrays = S.bunny_scene(n=76)
    W, H = a.width, a.height
    pt = make(arrays, W, H, 1000)
    pt.render(4096)
    ref = pt.readRadiance()[..., :3].astype(np.float64)
    pt.close()
    rows = []
    for thr in [float(x) for x in a.thresholds.split(",")]:
        acc = {"ad_err": [], "un_err": [], "k": [], "spp": [], "ad_gs": [], "un_gs": [], "min_share": [], "max_share": []}
        for s in range(SEEDS):
            pt = make(arrays, W, H, s)
            pt.render(a.round_ticks)  # (warm: code objects, the path state of a round)
            pt.clear()
            pt.seed(s + 1)
            t_ad = timed(pt, lambda: pt.render_adaptive(thr, max_ticks=a.max_ticks, min_ticks=a.min_ticks, round_ticks=a.round_ticks))
            st = pt.adaptive_stats()
            img_ad = pt.readRadiance()
            pt.close()
            k = max(1, int(round(st["samples"] / (W * H))))
            pu = make(arrays, W, H, s)
            pu.render(min(k, 128))  # (the path state of render(k)'s batches)
            pu.clear()
            pu.seed(s + 1)
            t_un = timed(pu, lambda: pu.render(k))
            img_un = pu.readRadiance()
            pu.close()
            e_ad, e_un = rel_mse(img_ad, ref), rel_mse(img_un, ref)
            tt = st["tile_ticks"][st["tile_ticks"] > 0]
            acc["ad_err"].append(e_ad); acc["un_err"].append(e_un); acc["k"].append(k)
            acc["spp"].append(st["samples"] / (W * H))
            acc["ad_gs"].append(st["samples"] / t_ad / 1e9); acc["un_gs"].append(W * H * k / t_un / 1e9)
            acc["min_share"].append(float((tt == a.min_ticks).mean())); acc["max_share"].append(float((tt == a.max_ticks).mean()))
        r = {"threshold": thr, **{key: float(np.mean(v)) for key, v in acc.items()}}
        r["ad_gs"], r["un_gs"] = float(np.median(acc["ad_gs"])), float(np.median(acc["un_gs"]))  # (rates: medians over seeds)
        spp_time = r["spp"] * r["un_gs"] / r["ad_gs"]  # uniform spp in the adaptive call's wall time
        r["un_err_time"] = r["un_err"] * r["k"] / spp_time
        r["equal_samples_ratio"] = r["ad_err"] / r["un_err"]
        r["equal_time_ratio"] = r["ad_err"] / r["un_err_time"]
        rows.append(r)
        print("threshold %.0e: %.1f spp avg (min-tick tiles %.0f %%, max-tick %.0f %%) | relMSE adaptive %.4g, uniform equal samples %.4g "
              "(x%.3f), equal time %.4g (x%.3f) | Gsamples/s adaptive %.3f, render(k) %.3f" %
              (thr, r["spp"], 100 * r["min_share"], 100 * r["max_share"], r["ad_err"], r["un_err"], r["equal_samples_ratio"],
               r["un_err_time"], r["equal_time_ratio"], r["ad_gs"], r["un_gs"]), flush=True)
    if a.out:
        json.dump({"width": W, "height": H, "max_ticks": a.max_ticks, "min_ticks": a.min_ticks, "round_ticks": a.round_ticks,
                   "seeds": SEEDS, "rows": rows}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
