#!/usr/bin/env python3
"""Interactive loop of the reference (main.js:838-857: tick() draws every frame) on C2 - the bunny scene at 1920x1080,
depth 8 - in three forms, interleaved on one box, --reps times:
    present: --frames x [tick(); present()]   (fspt_present: the frame of the previous call, one frame of latency)
    draw:    --frames x [tick(); draw()]      (fspt_draw_scaled into a preallocated buffer: what hosts do today)
    sync:    --frames x [tick(); sync()]      (bench.py's extra_configs.tick1: nothing drawn)
Each form gets --warmup frames first; every timed region ends with sync(), so each form's last frame is finished.
Prints one JSON line: ms per frame per form and repetition, and `equal` - the present target's final accumulator
against a render(n) of the same seed (whole frame, ==), and one intermediate presented frame against oracle.draw of the
oracle's accumulator at its tick, on a uniform sample of 32x32 tiles (bench.py parity_check's sampling).  The oracle
runs outside the timed regions.
usage: python tools/present_bench.py [--reps 3] [--frames 128] [--warmup 8]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import numpy as np  # noqa: E402

import fspt_amd  # noqa: E402
from fspt_amd import _lib as L, scene as S, distributed as D  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--warmup", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--bounces", type=int, default=8)
    ap.add_argument("--check-tick", type=int, default=3, help="ticks in the presented frame checked against the oracle")
    a = ap.parse_args()
    W, H, B = a.width, a.height, a.bounces
    arrays = S.bunny_scene(n=76, sun_deg=1.5, sun_gain=60.0)  # bench.py's C2
    cam = dict(S.BUNNY_CAMERA)
    lens = S.lens_features(cam["focal_depth"], cam["aperture"])

    def make():
        pt = fspt_amd.PathTracer(arrays, W, H, num_bounces=B)
        pt.set_camera(**cam)
        # (the default batch size: a target that only ever sees one-tick calls holds one tick of path state.  Not
        # set_pipeline(.., 1) as bench.py --tick-mode does: with a batch of one every recorded tick is flushed - a join -
        # at once, and present has nothing left to overlap)
        return pt

    pts = {f: make() for f in ("present", "draw", "sync")}
    out_buf = np.zeros((H, W, 4), np.uint8)
    lib = L.lib()

    def step(form, pt):
        pt.tick()
        if form == "present":
            return pt.present(out=out_buf)
        if form == "draw":
            L.check(lib.fspt_draw_scaled(pt._t, 1.0, 1.0, 0, 3.0, 1.0, L.u8ptr(out_buf)))
        else:
            pt.sync()
        return None

    ms = {f: [] for f in pts}
    checked = None
    for rep in range(a.reps):
        for form, pt in pts.items():
            pt.clear(); pt.seed(1); pt.sync()
            for k in range(a.warmup):
                r = step(form, pt)
                if form == "present" and rep == 0 and r is not None and r[1] == a.check_tick:
                    checked = r[0].copy()
            pt.sync()
            t0 = time.perf_counter()
            for _ in range(a.frames):
                step(form, pt)
            pt.sync()
            ms[form].append((time.perf_counter() - t0) * 1e3 / a.frames)

    # checks (untimed): the present target's accumulator after warmup + frames ticks against render(n) of the same seed
    n = a.warmup + a.frames
    got = pts["present"].readRadiance()
    for pt in pts.values():
        pt.close()
    ref = make(); ref.seed(1); ref.render(n)
    equal_final = bool(np.array_equal(got, ref.readRadiance()))
    ref.close()
    import oracle as O
    n_shards = max(1, int(-(-float(W) * H * a.check_tick // 3.0e7)))
    want = np.zeros((H, W, 4), np.float32)
    O.render(arrays, W, H, cam["P"], cam["I"], cam["fov_scale"], lens, cam["env_theta"], B, 0, a.check_tick, 1, want,
             shard=0, n_shards=n_shards, tile=D.TILE)
    mask = D.owner_mask(0, n_shards, W, H)
    owant = O.draw(want)
    equal_frame = checked is not None and bool(np.array_equal(checked[mask], owant[mask]))
    twin = make(); twin.seed(1)
    for _ in range(a.check_tick):
        twin.tick()
    gdraw = twin.draw()
    twin.close()
    diag = {"frame_vs_oracle_bad_px": None if checked is None else int((checked[mask] != owant[mask]).any(-1).sum()),
            "frame_vs_gpu_draw_bad_px": None if checked is None else int((checked != gdraw).any(-1).sum()),
            "gpu_draw_vs_oracle_bad_px": int((gdraw[mask] != owant[mask]).any(-1).sum())}
    res = {"workload": f"C2 {W}x{H} depth {B}: {a.frames} x [tick(); <form>] after {a.warmup} warm-up frames, interleaved",
           "reps": a.reps,
           "ms_per_frame": {f: [round(v, 4) for v in ms[f]] for f in ms},
           "present_below_draw_every_rep": all(p < d for p, d in zip(ms["present"], ms["draw"])),
           "equal": equal_final and equal_frame, "equal_final_vs_render": equal_final,
           "equal_frame_vs_oracle": equal_frame,
           "diag": diag,
           "frame_check": f"the frame of {a.check_tick} ticks, every {n_shards}-th 32x32 tile ({int(mask.sum())} pixels)"}
    print(json.dumps(res), flush=True)
    return 0 if res["equal"] else 1


if __name__ == "__main__":
    sys.exit(main())
