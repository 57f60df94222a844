"""Quality and cost of temporal accumulation: what fspt_temporal_accumulate buys a host whose picture changes.

  camera sequence     the medium test scene at 320 x 240; the camera orbits the scene's vertical axis by STEP degrees per
                      frame for F frames of n spp; relative MSE (error^2 / (reference^2 + 0.01)) of the LAST
                      frame against 4 096 spp from that camera: the raw frame, the temporal frame, temporal + a-trous,
                      a-trous alone
  parameter scan      the same sequence over a small grid of depth_tol, normal_cos, max_history
  geometry sequence   fixed camera, tests/refit_moves.py's rotation (7 degrees) reached in F equal steps through
                      update_geometry: with the motion origin (motion_begin before every update) and without it
  timing              both passes at 1920 x 1080 (HIP events) beside a one-sample fspt_features (host clock around a
                      synchronised call, best of 5) and the same host clock around a whole accumulate, in the same process; the snap's margin

usage: python tools/temporal_quality.py [--scan] [--timing]
tests/test_temporal_gpu.py::test_quality runs the two sequences and holds them to MEASURED x 1.5."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

W, H, FRAMES, SPP, STEP_DEG, GT_SPP, ATROUS = 320, 240, 8, 4, 2.0, 4096, 4
# ratios to the raw last frame measured on the MI355X with the shipped defaults (DESIGN 8.8 has the table)
MEASURED = {"camera_temporal_over_raw": 0.2025, "camera_temporal_atrous_over_raw": 0.0023, "geometry_with_origin_over_raw": 0.0350}


def rel_mse(x, gt):
    e = (x[..., :3].astype(np.float64) - gt[..., :3]) ** 2 / (gt[..., :3].astype(np.float64) ** 2 + 1e-2)
    return float(e.mean())


def orbit(camera, deg):
    th = np.radians(deg)
    R = np.array([[np.cos(th), 0, np.sin(th)], [0, 1, 0], [-np.sin(th), 0, np.cos(th)]])
    c = dict(camera)
    c["P"] = list(R @ np.array(camera["P"], np.float64))
    c["I"] = list(R @ np.array(camera["I"], np.float64))
    return c


def set_cam(pt, c):
    pt.set_camera(c["P"], c["I"], c["fov_scale"], c["env_theta"], c["focal_depth"], c["aperture"])


def reference(pt, seed=101):
    pt.clear(); pt.seed(seed); pt.render(GT_SPP)
    return pt.readRadiance()


def camera_sequence(arrays, camera, params=None, frames=FRAMES, spp=SPP, gt=None):
    from fspt_amd import PathTracer
    params = params or {}
    pt = PathTracer(arrays, W, H, num_bounces=4)
    last = orbit(camera, STEP_DEG * (frames - 1))
    set_cam(pt, last)
    if gt is None:
        gt = reference(pt)
    for k in range(frames):
        set_cam(pt, orbit(camera, STEP_DEG * k))
        pt.clear(); pt.seed(7 + k); pt.render(spp)
        hist = pt.temporal_accumulate(**params)
    raw = pt.readRadiance()
    pt.features(8, 1)
    out = {"raw": rel_mse(raw, gt), "temporal": rel_mse(hist, gt), "temporal_atrous": rel_mse(pt.temporal_denoise(iterations=ATROUS), gt),
           "atrous": rel_mse(pt.denoise(iterations=ATROUS), gt), "mean_length": float(hist[..., 3].mean()), "gt": gt}
    pt.close(); pt.scene.close()
    return out


def geometry_sequence(arrays, camera, params=None, frames=FRAMES, spp=SPP):
    from fspt_amd import PathTracer
    from refit_moves import rotated
    params = params or {}
    out = {}
    for origin in (True, False):
        pt = PathTracer(arrays, W, H, num_bounces=4)
        set_cam(pt, camera)
        for k in range(frames):
            if k:
                if origin:
                    pt.scene.motion_begin()
                pt.update_geometry(*rotated(arrays.tri, arrays.norm, deg=7.0 * k / (frames - 1)))
            pt.clear(); pt.seed(7 + k); pt.render(spp)
            hist = pt.temporal_accumulate(**params)
        raw = pt.readRadiance()
        if "gt" not in out:
            out["gt"] = reference(pt)
        out["raw"] = rel_mse(raw, out["gt"])
        out["with_origin" if origin else "without_origin"] = rel_mse(hist, out["gt"])
        pt.close(); pt.scene.close()
    del out["gt"]
    return out


def timing(arrays, camera, w=1920, h=1080):
    from fspt_amd import PathTracer
    pt = PathTracer(arrays, w, h, num_bounces=4)
    set_cam(pt, camera)
    pt.render(1)
    best = [1e9, 1e9]
    for k in range(6):
        set_cam(pt, orbit(camera, 0.5 * k))
        pt.temporal_accumulate(read=False)
        ms = pt.temporal_last_ms()
        if k:
            best = [min(a, b) for a, b in zip(best, ms)]
    host = 1e9
    for k in range(6):
        set_cam(pt, orbit(camera, 0.5 * k))
        pt.sync()
        t0 = time.perf_counter()
        pt.temporal_accumulate(read=False); pt.sync()
        if k:
            host = min(host, (time.perf_counter() - t0) * 1e3)
    feat = 1e9
    for k in range(6):
        pt.sync()
        t0 = time.perf_counter()
        pt.features(1, 1 + k); pt.sync()
        if k:
            feat = min(feat, (time.perf_counter() - t0) * 1e3)
    pt.close(); pt.scene.close()
    return {"gbuffer_motion_ms": best[0], "blend_ms": best[1], "accumulate_host_ms": host, "features_1spp_host_ms": feat}


def snap_margin(arrays, camera, w=1920, h=1080):
    """How far a STATIC view's unsnapped sample positions lie from the pixel they belong to (the float32 error the 1/128-pixel
    snap has to cover): tests/temporal_ref.py's float64 projection of the GPU's own float32 G, at the test camera and from
    8 x as far away with 1/8 of the field of view (the same picture, 8 x the magnitudes)."""
    import temporal_ref as T
    from fspt_amd import PathTracer
    out = {}
    for name, far in (("near", 1.0), ("far_x8", 8.0)):
        c = dict(camera)
        c["P"] = [far * x for x in camera["P"]]
        c["fov_scale"] = camera["fov_scale"] / far
        pt = PathTracer(arrays, w, h, num_bounces=4)
        set_cam(pt, c)
        pt.render(1)
        pt.temporal_accumulate(read=False)
        pt.temporal_accumulate(read=False)
        G, M = pt.temporal_gbuffer()
        _, d = T.centre_rays(w, h, c["P"], c["I"], c["fov_scale"])
        cam = (c["P"], c["I"], c["fov_scale"])
        m = T.motion(G, d, cam, cam)
        xs, ys = np.meshgrid(np.arange(w), np.arange(h))
        out[name] = {"worst_px": float(max(np.abs(m["sx_raw"] - xs).max(), np.abs(m["sy_raw"] - ys).max())),
                     "snapped_all": bool(np.array_equal(M[..., 0], xs) and np.array_equal(M[..., 1], ys))}
        pt.close(); pt.scene.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scan", action="store_true")
    ap.add_argument("--timing", action="store_true")
    args = ap.parse_args()
    from fspt_amd import scene as S
    arrays = S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0)  # the tests' medium scene
    cam = dict(S.BUNNY_CAMERA)
    q = camera_sequence(arrays, cam)
    gt = q.pop("gt")
    print("camera sequence (defaults):", {k: round(v, 5) for k, v in q.items()})
    print("  ratios to raw: temporal %.4f  temporal+atrous %.4f  atrous alone %.4f" %
          (q["temporal"] / q["raw"], q["temporal_atrous"] / q["raw"], q["atrous"] / q["raw"]))
    g = geometry_sequence(arrays, cam)
    print("geometry sequence (defaults):", {k: round(v, 5) for k, v in g.items()})
    print("  ratios to raw: with origin %.4f  without %.4f" % (g["with_origin"] / g["raw"], g["without_origin"] / g["raw"]))
    if args.scan:
        print("| depth_tol | normal_cos | max_history | temporal / raw | temporal + a-trous / raw | mean length |")
        print("|---|---|---|---|---|---|")
        for dt in (0.02, 0.05, 0.1):
            for nc in (0.8, 0.9, 0.95):
                for mh in (16.0, 32.0, 64.0):
                    r = camera_sequence(arrays, cam, dict(depth_tol=dt, normal_cos=nc, max_history=mh), gt=gt)
                    print("| %g | %g | %g | %.4f | %.4f | %.1f |" % (dt, nc, mh, r["temporal"] / r["raw"], r["temporal_atrous"] / r["raw"], r["mean_length"]))
    if args.timing:
        print("timing 1920 x 1080:", {k: round(v, 4) for k, v in timing(arrays, cam).items()})
        print("snap margin 1920 x 1080 (1/128 = 0.0078):", snap_margin(arrays, cam))


if __name__ == "__main__":
    main()
