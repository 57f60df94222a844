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

  --variance          DESIGN 8.9: the variance-guided filter (fspt_temporal_denoise_variance) against fspt_temporal_denoise on the same
                      frames in the same process, each at its best scanned setting (VARIANCE_BEST / FIXED_BEST), on the two sequences
                      above and on the EDGE sequence - tests/lights_ref.py's scene E3 (an occluder under a lamp, emitters standing on
                      and facing the floor: shadow edges and thin bright shapes), 16 frames of 4 spp = 64 samples from a camera that
                      orbits 0.25 degrees per frame, so that most pixels keep a long history; with --scan the settings scanned; with
                      --timing the moments blend, k_svgf_variance and the guided iterations at 1920 x 1080 beside the parent's passes

  --clamp             DESIGN 8.10: the history clamp (fspt_temporal_set_clamp) off and on, from the same inputs in the same process, on
                      the LIGHT sequence - tests/lights_ref.py's scene E3 (it has an environment map) from a fixed camera, 16 frames
                      of 4 spp at env_theta t0, until the history is full, then 8 frames at t0 + 90 degrees; relative MSE of the last
                      frame against 4 096 spp at t0 + 90 - and, as the clamp's cost where the light is stable, on the camera sequence
                      above; with --scan sigma_scale {1, 2, 3, 4} x fast_history {8, 16, 32} on both; with --timing the blend pass with the mode off and on and k_temporal_clamp at 1920 x 1080

usage: python tools/temporal_quality.py [--scan] [--timing] [--variance | --clamp]
tests/test_temporal_gpu.py::test_quality runs the two sequences and holds them to MEASURED x 1.5."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fspt_amd import _lib as L  # noqa: E402

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


# ---- variance guidance --------------------------------------------------------------------------------------
EDGE_FRAMES, EDGE_SPP, EDGE_STEP_DEG = 16, 4, 0.25
FIXED_BEST = dict(iterations=4, sigma_color=4.0, sigma_normal=32.0, sigma_depth=0.05)      # the library's defaults; the comparison takes the minimum over FIXED_SCAN too
VARIANCE_BEST = dict(iterations=4, sigma_color=8.0, sigma_normal=32.0, sigma_depth=0.05)   # the library's defaults, chosen by DESIGN 8.9's scan on these same sequences
FIXED_SCAN = [dict(iterations=k, sigma_color=sc) for k in (3, 4, 5) for sc in (1.0, 2.0, 4.0, 8.0)]
VARIANCE_SCAN = [dict(iterations=k, sigma_color=sl) for k in (3, 4, 5) for sl in (1.0, 2.0, 4.0, 8.0, 16.0)]


def variance_sequence(arrays, camera, frames, spp, step_deg=0.0, geometry_deg=0.0, fixed=(FIXED_BEST,), variance=(VARIANCE_BEST,), gt=None):
    """One sequence with moments on (the colour history is the same bit for bit); after the last frame every setting of
    `fixed` through temporal_denoise and every setting of `variance` through temporal_denoise(variance=True), on that one
    history.  Returns relative MSEs of the last frame: raw, temporal, lists fixed / variance, and gt."""
    from fspt_amd import PathTracer
    from refit_moves import rotated
    pt = PathTracer(arrays, W, H, num_bounces=4)
    pt.temporal_set_moments(True)
    set_cam(pt, orbit(camera, step_deg * (frames - 1)))
    if gt is None:
        if geometry_deg:
            pt.update_geometry(*rotated(arrays.tri, arrays.norm, deg=geometry_deg))
        gt = reference(pt)
        if geometry_deg:
            pt.update_geometry(arrays.tri, arrays.norm)
    for k in range(frames):
        set_cam(pt, orbit(camera, step_deg * k))
        if k and geometry_deg:
            pt.scene.motion_begin()
            pt.update_geometry(*rotated(arrays.tri, arrays.norm, deg=geometry_deg * k / (frames - 1)))
        pt.clear(); pt.seed(7 + k); pt.render(spp)
        pt.features(8, 1)
        hist = pt.temporal_accumulate()
    out = {"raw": rel_mse(pt.readRadiance(), gt), "temporal": rel_mse(hist, gt), "gt": gt,
           "fixed": [rel_mse(pt.temporal_denoise(**q), gt) for q in fixed],
           "variance": [rel_mse(pt.temporal_denoise(variance=True, **q), gt) for q in variance]}
    pt.close(); pt.scene.close()
    return out


def variance_sequences(arrays, camera):
    """name -> (arrays, camera, keyword arguments of variance_sequence) of the three sequences"""
    import lights_ref as LR
    return {"camera": (arrays, camera, dict(frames=FRAMES, spp=SPP, step_deg=STEP_DEG)),
            "geometry": (arrays, camera, dict(frames=FRAMES, spp=SPP, geometry_deg=7.0)),
            "edges": (LR.scene_e3(), camera, dict(frames=EDGE_FRAMES, spp=EDGE_SPP, step_deg=EDGE_STEP_DEG))}


def variance_comparison(arrays, camera, scan=False):
    """name -> {raw, temporal, fixed, fixed_best, variance}: the fixed rule at the library's defaults and at the best of
    FIXED_SCAN FOR THAT SEQUENCE (it always runs its whole scan: the strongest opponent), the variance-guided filter at ONE
    setting, VARIANCE_BEST = the library's defaults (scan: also the lists fixed_scan / variance_scan)"""
    out = {}
    for name, (a, c, kw) in variance_sequences(arrays, camera).items():
        fx = [FIXED_BEST] + FIXED_SCAN
        vr = [VARIANCE_BEST] + (VARIANCE_SCAN if scan else [])
        r = variance_sequence(a, c, fixed=fx, variance=vr, **kw)
        out[name] = {"raw": r["raw"], "temporal": r["temporal"], "fixed": r["fixed"][0], "fixed_best": min(r["fixed"]), "variance": r["variance"][0]}
        if scan:
            out[name]["fixed_scan"], out[name]["variance_scan"] = r["fixed"][1:], r["variance"][1:]
    return out


def variance_timing(arrays, camera, w=1920, h=1080):
    """HIP-event ms, best of 5, in one process: the blend pass with moments off and on, the parent's filter (host clock around
    a synchronised temporal_denoise: it has no events of its own; the guided one the same way beside its events), k_svgf_variance
    on a first frame (every pixel takes the 7 x 7 window) and on a long history (none does)."""
    from fspt_amd import PathTracer
    pt = PathTracer(arrays, w, h, num_bounces=4)
    set_cam(pt, camera)
    pt.render(1); pt.features(1, 1)
    out = {}

    def host(fn):
        best = 1e9
        for _ in range(6):
            pt.sync(); t0 = time.perf_counter(); fn(); pt.sync()
            best = min(best, (time.perf_counter() - t0) * 1e3)
        return best
    for on in (False, True):
        pt.temporal_set_moments(on)
        best = 1e9
        for k in range(6):
            pt.temporal_accumulate(read=False)
            if k:
                best = min(best, pt.temporal_last_ms()[1])
        out["blend_moments_%s_ms" % ("on" if on else "off")] = best
    pt.temporal_reset(); pt.temporal_accumulate(read=False)
    for name in ("first_frame", "long_history"):
        if name == "long_history":
            for _ in range(6):
                pt.temporal_accumulate(read=False)
        bv, bi = 1e9, 1e9
        for k in range(6):
            L.check(L.lib().fspt_temporal_denoise_variance(pt._t, None, None))
            ms = pt.svgf_last_ms()
            if k:
                bv, bi = min(bv, ms[0]), min(bi, ms[1])
        out["svgf_variance_%s_ms" % name], out["guided_4_iterations_%s_ms" % name] = bv, bi
    out["guided_host_ms"] = host(lambda: L.check(L.lib().fspt_temporal_denoise_variance(pt._t, None, None)))
    out["fixed_4_iterations_host_ms"] = host(lambda: L.check(L.lib().fspt_temporal_denoise(pt._t, None, None)))
    pt.close(); pt.scene.close()
    return out


# ---- history clamp -----------------------------------------------------------------------------------------
LIGHT_BEFORE, LIGHT_AFTER, LIGHT_DEG = 16, 8, 90.0
CLAMP_BEST = dict(fast_history=32.0, sigma_scale=1.0)  # the library's defaults (DESIGN 8.10's scan)
CLAMP_SCAN = [dict(fast_history=float(f), sigma_scale=float(s)) for s in (1, 2, 3, 4) for f in (8, 16, 32)]
# on / off of the LIGHT sequence's last frame measured on the MI355X with the shipped defaults (DESIGN 8.10 has the table)
CLAMP_MEASURED = {"light_on_over_off": 0.557}


def light_sequence(arrays, camera, settings, step_deg=0.0, before=LIGHT_BEFORE, after_frames=LIGHT_AFTER, gt=None):
    """One sequence per entry of `settings` (None = the clamp off, else temporal_set_clamp's parameters), all from the same
    frames: LIGHT_BEFORE frames, then the change (env_theta + LIGHT_DEG), then LIGHT_AFTER frames.  step_deg != 0: no change
    of light, the camera orbits instead (the clamp's cost).  -> ([rel MSE of the last frame], raw, gt)"""
    from fspt_amd import PathTracer
    frames = before + after_frames
    after = dict(camera) if step_deg else dict(camera, env_theta=camera["env_theta"] + np.radians(LIGHT_DEG))
    pts = []
    for q in settings:
        pt = PathTracer(arrays, W, H, num_bounces=4)
        if q is not None:
            pt.temporal_set_clamp(True, **q)
        pts.append(pt)
    if gt is None:
        pt = pts[0]
        set_cam(pt, orbit(after, step_deg * (frames - 1)))
        gt = reference(pt)
    res, raw = [], None
    for pt in pts:
        for k in range(frames):
            changed = k >= before
            set_cam(pt, orbit(after if changed else camera, step_deg * k))
            pt.clear(); pt.seed(7 + k); pt.render(SPP)
            hist = pt.temporal_accumulate()
        res.append(rel_mse(hist, gt))
        raw = rel_mse(pt.readRadiance(), gt)
        pt.close(); pt.scene.close()
    return res, raw, gt


def clamp_comparison(camera, scan=False, cost_arrays=None):
    """name -> {raw, off, on[, scan]}: "light" always; "camera" - DESIGN 8.8's camera sequence on cost_arrays, where the light
    is stable and the clamp can only cost - on request"""
    import lights_ref as LR
    settings = [None, CLAMP_BEST] + (CLAMP_SCAN if scan else [])
    out = {}
    for name, a, kw in (("light", LR.scene_e3(), {}), ("camera", cost_arrays, dict(step_deg=STEP_DEG, before=FRAMES, after_frames=0))):
        if a is None:
            continue
        r, raw, _ = light_sequence(a, camera, settings, **kw)
        out[name] = {"raw": raw, "off": r[0], "on": r[1]}
        if scan:
            out[name]["scan"] = r[2:]
    return out


def clamp_timing(arrays, camera, w=1920, h=1080):
    """HIP-event ms, best of 5 after a warm-up, in one process: the blend pass with the mode off and on, k_temporal_clamp"""
    from fspt_amd import PathTracer
    pt = PathTracer(arrays, w, h, num_bounces=4)
    set_cam(pt, camera)
    pt.render(1)
    out = {}
    for on in (False, True):
        pt.temporal_set_clamp(on)
        bb, bc = 1e9, 1e9
        for k in range(6):
            pt.temporal_accumulate(read=False)
            if k:
                bb = min(bb, pt.temporal_last_ms()[1])
                if on:
                    bc = min(bc, pt.temporal_clamp_last_ms())
        out["blend_clamp_%s_ms" % ("on" if on else "off")] = bb
        if on:
            out["temporal_clamp_ms"] = bc
    pt.close(); pt.scene.close()
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
    ap.add_argument("--variance", action="store_true", help="the variance-guided filter against the fixed rule (DESIGN 8.9)")
    ap.add_argument("--clamp", action="store_true", help="the history clamp off and on over a change of light (DESIGN 8.10)")
    args = ap.parse_args()
    from fspt_amd import scene as S
    arrays = S.bunny_scene(n=24, env_size=(256, 128), sun_deg=3.0)  # the tests' medium scene
    cam = dict(S.BUNNY_CAMERA)
    if args.clamp:
        r = clamp_comparison(cam, scan=args.scan, cost_arrays=arrays)
        print("| sequence | raw last frame | clamp off | clamp on (defaults) | on / off |")
        print("|---|---|---|---|---|")
        for name, v in r.items():
            print("| %s | %.5f | %.5f | %.5f | %.3f |" % (name, v["raw"], v["off"], v["on"], v["on"] / v["off"]))
        if args.scan:
            for name, v in r.items():
                print(name, "scan:", " ".join("s%g/f%g:%.5f" % (q["sigma_scale"], q["fast_history"], x) for q, x in zip(CLAMP_SCAN, v["scan"])))
        if args.timing:
            print("clamp timing 1920 x 1080:", {k: round(v, 4) for k, v in clamp_timing(arrays, cam).items()})
        return
    if args.variance:
        r = variance_comparison(arrays, cam, scan=args.scan)
        print("| sequence | raw | temporal | + a-trous, fixed rule (defaults) | fixed rule (its best scanned row) | + variance-guided a-trous (defaults) | guided / best fixed |")
        print("|---|---|---|---|---|---|---|")
        for name, v in r.items():
            print("| %s | %.5f | %.5f | %.5f | %.5f | %.5f | %.3f |" % (name, v["raw"], v["temporal"], v["fixed"], v["fixed_best"], v["variance"], v["variance"] / v["fixed_best"]))
        if args.scan:
            for name, v in r.items():
                print(name, "fixed rule:", " ".join("K%d/sc%g:%.5f" % (q["iterations"], q["sigma_color"], x) for q, x in zip(FIXED_SCAN, v["fixed_scan"])))
                print(name, "variance-guided:", " ".join("K%d/sl%g:%.5f" % (q["iterations"], q["sigma_color"], x) for q, x in zip(VARIANCE_SCAN, v["variance_scan"])))
        if args.timing:
            print("variance timing 1920 x 1080:", {k: round(v, 4) for k, v in variance_timing(arrays, cam).items()})
        return
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
